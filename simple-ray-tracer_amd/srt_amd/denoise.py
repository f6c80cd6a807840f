"""The edge-avoiding denoiser for progressive frames (include/srt_denoise.h), guided by ray queries.

``Denoiser(width, height)`` allocates its device buffers once.  ``primary_rays(camera)`` writes the pixel-centre
camera rays into a device tensor; ``Query.closest`` of those rays is the guide; ``run(accum, frames, hits)``
filters the accumulation image (a torch tensor, or the raw device pointer ``Compute.image_pointers()``
returns) and returns device tensors.  Nothing leaves the device and no call synchronises.  Full frames only.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import DenoiseParams, DenoiseVarParams, check, lib

__all__ = ["Denoiser", "ALBEDO_FLOOR"]

# run_albedo's default floor (the C ABI has none): chosen on the CPU by tools/albedo_floor_grid.py (DESIGN.md
# section 5, "Surface attributes and demodulation"); srt::kAlbedoFloor in include/srt/denoise.hpp is the same.
ALBEDO_FLOOR = 0.1


class Denoiser:
    """A denoiser for ``width`` x ``height`` frames on ``device``.

    ``stream``: a ``torch.cuda.Stream`` or a raw ``hipStream_t`` handle.  With the default (None) the object runs
    on a stream of its own and orders every call with ``torch.cuda.current_stream()`` by events, exactly as
    :class:`srt_amd.query.Query` does.
    """

    def __init__(self, width: int, height: int, device: int = 0, stream=None):
        self.width, self.height, self.device = int(width), int(height), int(device)
        self._d = None
        self._ext = None
        handle = getattr(stream, "cuda_stream", stream)
        self._own_stream = not handle
        h = C.c_void_p()
        check(lib().srt_denoise_create(self.device, C.c_void_p(handle) if handle else None, self.width, self.height,
                                       C.byref(h)), "srt_denoise_create")
        self._d = h

    # -- lifecycle ------------------------------------------------------------
    def close(self):
        if self._d is not None:
            lib().srt_denoise_destroy(self._d)
            self._d = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @property
    def handle(self):
        if self._d is None:
            raise RuntimeError("Denoiser is closed")
        return self._d

    # -- state ----------------------------------------------------------------
    def get_int(self, name: str) -> int:
        v = C.c_int()
        check(lib().srt_denoise_get_int(self.handle, name.encode(), C.byref(v)), f"srt_denoise_get_int({name})")
        return v.value

    @property
    def params(self) -> dict:
        p = DenoiseParams()
        check(lib().srt_denoise_get_params(self.handle, C.byref(p)), "srt_denoise_get_params")
        return {n: getattr(p, n) for n, _ in DenoiseParams._fields_}

    def set_params(self, **kw):
        """Any of passes, normal_squarings, sigma_color, sigma_depth; the others keep their values."""
        cur = self.params
        unknown = set(kw) - set(cur)
        if unknown:
            raise TypeError(f"unknown denoiser parameter(s): {sorted(unknown)}")
        cur.update(kw)
        p = DenoiseParams(int(cur["passes"]), int(cur["normal_squarings"]), float(cur["sigma_color"]),
                          float(cur["sigma_depth"]))
        check(lib().srt_denoise_set_params(self.handle, C.byref(p)), "srt_denoise_set_params")

    # -- work -----------------------------------------------------------------
    def _ordered(self, torch):
        if not self._own_stream:
            return None
        if self._ext is None:
            self._ext = torch.cuda.ExternalStream(int(lib().srt_denoise_stream(self.handle)), device=self.device)
        return self._ext

    def _run(self, call, what):
        import torch
        ext = self._ordered(torch)
        cur = torch.cuda.current_stream(self.device) if ext is not None else None
        if ext is not None:
            ext.wait_stream(cur)
        check(call(), what)
        if ext is not None:
            cur.wait_stream(ext)

    def primary_rays(self, camera):
        """The pixel-centre rays of ``camera`` (getOrigin / getForward / getRightVector / getUpVector) as a
        device ``[W * H, 8]`` float32 tensor of ``srt_ray`` records, index ``j * W + i``, row 0 at the bottom."""
        import torch
        vec = [np.ascontiguousarray(np.asarray(v, np.float32).reshape(3)) for v in
               (camera.getOrigin(), camera.getForward(), camera.getRightVector(), camera.getUpVector())]
        rays = torch.empty((self.width * self.height, 8), dtype=torch.float32, device=f"cuda:{self.device}")
        self._run(lambda: lib().srt_denoise_primary_rays(self.handle, *[C.c_void_p(v.ctypes.data) for v in vec],
                                                         C.c_void_p(rays.data_ptr())), "srt_denoise_primary_rays")
        return rays

    def run(self, accum, frames: int, hits=None, *, srgb: bool = False):
        """Filter the accumulation image ``accum`` (the SUM over ``frames``): a contiguous float32 ``[H, W, 4]``
        device tensor, or a raw device pointer (int).  ``hits``: the guide, a :class:`srt_amd.query.Hits` or its
        ``[W * H, 8]`` int32 tensor (may be None when passes == 0).  Returns the float32 ``[H, W, 4]`` result on
        the device, and with ``srgb=True`` the pair (float32 image, uint8 ``[H, W, 4]`` sRGB image)."""
        import torch
        dev = f"cuda:{self.device}"
        if isinstance(accum, int):
            acc_ptr, keep = accum, None
        else:
            if (accum.dtype != torch.float32 or not accum.is_cuda or accum.device.index != self.device
                    or not accum.is_contiguous() or accum.numel() != self.width * self.height * 4):
                raise ValueError(f"accum must be a contiguous float32 [H, W, 4] tensor on {dev}")
            acc_ptr, keep = accum.data_ptr(), accum
        raw = getattr(hits, "raw", hits)
        if raw is not None and (raw.dtype != torch.int32 or not raw.is_cuda or raw.device.index != self.device
                                or not raw.is_contiguous() or tuple(raw.shape) != (self.width * self.height, 8)):
            raise ValueError(f"hits must be the [W * H, 8] int32 srt_hit tensor on {dev}")
        out = torch.empty((self.height, self.width, 4), dtype=torch.float32, device=dev)
        out8 = torch.empty((self.height, self.width, 4), dtype=torch.uint8, device=dev) if srgb else None
        self._run(lambda: lib().srt_denoise_run(self.handle, C.c_void_p(acc_ptr), int(frames),
                                                C.c_void_p(raw.data_ptr()) if raw is not None else None,
                                                C.c_void_p(out.data_ptr()),
                                                C.c_void_p(out8.data_ptr()) if srgb else None), "srt_denoise_run")
        del keep
        return (out, out8) if srgb else out

    # -- the variance-guided filter (include/srt_variance.h) --------------------
    def enable_variance(self):
        """Allocate the ping-pong variance arrays; idempotent."""
        check(lib().srt_denoise_enable_variance(self.handle), "srt_denoise_enable_variance")

    @property
    def variance_params(self) -> dict:
        p = DenoiseVarParams()
        check(lib().srt_denoise_get_var_params(self.handle, C.byref(p)), "srt_denoise_get_var_params")
        return {n: getattr(p, n) for n, _ in DenoiseVarParams._fields_}

    def set_variance_params(self, **kw):
        """Any of sigma_lum, min_history; the other keeps its value."""
        cur = self.variance_params
        unknown = set(kw) - set(cur)
        if unknown:
            raise TypeError(f"unknown variance parameter(s): {sorted(unknown)}")
        cur.update(kw)
        mh = int(cur["min_history"])
        if not 0 <= mh <= 0xFFFFFFFF:
            raise ValueError("min_history must fit an unsigned 32-bit integer")
        p = DenoiseVarParams(float(cur["sigma_lum"]), mh)
        check(lib().srt_denoise_set_var_params(self.handle, C.byref(p)), "srt_denoise_set_var_params")

    def run_variance(self, colour, frames: int, hits, moments, *, srgb: bool = False):
        """The variance-guided filter: ``colour`` (the SUM over ``frames``; ``Temporal.accumulate_moments``' ``out``
        with ``frames`` = 1) and ``moments`` are contiguous float32 ``[H, W, 4]`` device tensors, ``hits`` the guide.
        Uses ``passes`` (at least 1), ``normal_squarings`` and ``sigma_depth`` of ``params`` and ``variance_params``.
        Returns ``(out, variance)``: the float32 ``[H, W, 4]`` result and the float32 ``[H, W]`` variance left after
        the last pass; with ``srgb=True`` ``(out, out8, variance)``.  Needs ``enable_variance()``."""
        import torch
        dev = f"cuda:{self.device}"
        for name, t in (("colour", colour), ("moments", moments)):
            if (t.dtype != torch.float32 or not t.is_cuda or t.device.index != self.device
                    or not t.is_contiguous() or t.numel() != self.width * self.height * 4):
                raise ValueError(f"{name} must be a contiguous float32 [H, W, 4] tensor on {dev}")
        raw = getattr(hits, "raw", hits)
        if raw is None or (raw.dtype != torch.int32 or not raw.is_cuda or raw.device.index != self.device
                           or not raw.is_contiguous() or tuple(raw.shape) != (self.width * self.height, 8)):
            raise ValueError(f"hits must be the [W * H, 8] int32 srt_hit tensor on {dev}")
        out = torch.empty((self.height, self.width, 4), dtype=torch.float32, device=dev)
        out8 = torch.empty((self.height, self.width, 4), dtype=torch.uint8, device=dev) if srgb else None
        var = torch.empty((self.height, self.width), dtype=torch.float32, device=dev)
        self._run(lambda: lib().srt_denoise_run_variance(self.handle, C.c_void_p(colour.data_ptr()), int(frames),
                                                         C.c_void_p(raw.data_ptr()), C.c_void_p(moments.data_ptr()),
                                                         C.c_void_p(out.data_ptr()),
                                                         C.c_void_p(out8.data_ptr()) if srgb else None,
                                                         C.c_void_p(var.data_ptr())), "srt_denoise_run_variance")
        return (out, out8, var) if srgb else (out, var)

    # -- albedo-demodulated filtering (include/srt_surface.h) -------------------
    def run_albedo(self, accum, frames: int, hits, attrs, albedo_floor: float = ALBEDO_FLOOR, *, srgb: bool = False):
        """``run`` on radiance divided by the surface albedo: ``attrs`` is ``Surface.shade``'s float32
        ``[W * H, 8]`` tensor for the pixel-centre rays (may be None when passes == 0).  A hit pixel's mean is
        divided by ``max(albedo, albedo_floor)`` before the first pass and the filtered colour multiplied by it in
        the last; miss pixels pass through.  Same arguments and results as ``run`` otherwise."""
        import torch
        dev = f"cuda:{self.device}"
        if isinstance(accum, int):
            acc_ptr, keep = accum, None
        else:
            if (accum.dtype != torch.float32 or not accum.is_cuda or accum.device.index != self.device
                    or not accum.is_contiguous() or accum.numel() != self.width * self.height * 4):
                raise ValueError(f"accum must be a contiguous float32 [H, W, 4] tensor on {dev}")
            acc_ptr, keep = accum.data_ptr(), accum
        raw = getattr(hits, "raw", hits)
        if raw is not None and (raw.dtype != torch.int32 or not raw.is_cuda or raw.device.index != self.device
                                or not raw.is_contiguous() or tuple(raw.shape) != (self.width * self.height, 8)):
            raise ValueError(f"hits must be the [W * H, 8] int32 srt_hit tensor on {dev}")
        if attrs is not None and (attrs.dtype != torch.float32 or not attrs.is_cuda or attrs.device.index != self.device
                                  or not attrs.is_contiguous() or tuple(attrs.shape) != (self.width * self.height, 8)):
            raise ValueError(f"attrs must be the [W * H, 8] float32 srt_surface_attr tensor on {dev}")
        out = torch.empty((self.height, self.width, 4), dtype=torch.float32, device=dev)
        out8 = torch.empty((self.height, self.width, 4), dtype=torch.uint8, device=dev) if srgb else None
        self._run(lambda: lib().srt_denoise_run_albedo(self.handle, C.c_void_p(acc_ptr), int(frames),
                                                       C.c_void_p(raw.data_ptr()) if raw is not None else None,
                                                       C.c_void_p(attrs.data_ptr()) if attrs is not None else None,
                                                       C.c_float(albedo_floor), C.c_void_p(out.data_ptr()),
                                                       C.c_void_p(out8.data_ptr()) if srgb else None),
                  "srt_denoise_run_albedo")
        del keep
        return (out, out8) if srgb else out

    def synchronize(self):
        """Wait for the work enqueued so far."""
        import torch
        torch.cuda.ExternalStream(int(lib().srt_denoise_stream(self.handle) or 0), device=self.device).synchronize()
