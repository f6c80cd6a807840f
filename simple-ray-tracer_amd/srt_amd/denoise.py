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
from ._stage import _Stage, accum_arg, attrs_arg, get_params, hits_arg, image_arg, updated_params

__all__ = ["Denoiser", "ALBEDO_FLOOR"]

# run_albedo's default floor (the C ABI has none): chosen on the CPU by tools/albedo_floor_grid.py (DESIGN.md
# section 5, "Surface attributes and demodulation"); srt::kAlbedoFloor in include/srt/denoise.hpp is the same.
ALBEDO_FLOOR = 0.1


class Denoiser(_Stage):
    """A denoiser for ``width`` x ``height`` frames on ``device``.

    ``stream``: a ``torch.cuda.Stream`` or a raw ``hipStream_t`` handle.  With the default (None) the object runs
    on a stream of its own and orders every call with ``torch.cuda.current_stream()`` by events, exactly as
    :class:`srt_amd.query.Query` does.
    """

    _prefix = "srt_denoise"

    def __init__(self, width: int, height: int, device: int = 0, stream=None):
        super().__init__(device, stream)
        self.width, self.height = int(width), int(height)
        self._create(self.width, self.height)

    # -- state ----------------------------------------------------------------
    @property
    def params(self) -> dict:
        return get_params(DenoiseParams, lib().srt_denoise_get_params, self.handle, "srt_denoise_get_params")

    def set_params(self, **kw):
        """Any of passes, normal_squarings, sigma_color, sigma_depth; the others keep their values."""
        p = updated_params(DenoiseParams, self.params, kw, "denoiser")
        check(lib().srt_denoise_set_params(self.handle, C.byref(p)), "srt_denoise_set_params")

    # -- work -----------------------------------------------------------------
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
        acc_ptr, keep = accum_arg(accum, self.width, self.height, self.device)
        hit_ptr, raw = hits_arg(hits, self.width * self.height, self.device, required=False)
        out = torch.empty((self.height, self.width, 4), dtype=torch.float32, device=dev)
        out8 = torch.empty((self.height, self.width, 4), dtype=torch.uint8, device=dev) if srgb else None
        self._run(lambda: lib().srt_denoise_run(self.handle, C.c_void_p(acc_ptr), int(frames), C.c_void_p(hit_ptr),
                                                C.c_void_p(out.data_ptr()),
                                                C.c_void_p(out8.data_ptr()) if srgb else None), "srt_denoise_run")
        del keep, raw
        return (out, out8) if srgb else out

    # -- the variance-guided filter (include/srt_variance.h) --------------------
    def enable_variance(self):
        """Allocate the ping-pong variance arrays; idempotent."""
        check(lib().srt_denoise_enable_variance(self.handle), "srt_denoise_enable_variance")

    @property
    def variance_params(self) -> dict:
        return get_params(DenoiseVarParams, lib().srt_denoise_get_var_params, self.handle, "srt_denoise_get_var_params")

    def set_variance_params(self, **kw):
        """Any of sigma_lum, min_history; the other keeps its value."""
        p = updated_params(DenoiseVarParams, self.variance_params, kw, "variance")
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
            image_arg(name, t, self.width, self.height, self.device)
        _, raw = hits_arg(hits, self.width * self.height, self.device)
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
        acc_ptr, keep = accum_arg(accum, self.width, self.height, self.device)
        hit_ptr, raw = hits_arg(hits, self.width * self.height, self.device, required=False)
        attr_ptr, _ = attrs_arg(attrs, self.width * self.height, self.device, required=False)
        out = torch.empty((self.height, self.width, 4), dtype=torch.float32, device=dev)
        out8 = torch.empty((self.height, self.width, 4), dtype=torch.uint8, device=dev) if srgb else None
        self._run(lambda: lib().srt_denoise_run_albedo(self.handle, C.c_void_p(acc_ptr), int(frames), C.c_void_p(hit_ptr),
                                                       C.c_void_p(attr_ptr), C.c_float(albedo_floor),
                                                       C.c_void_p(out.data_ptr()),
                                                       C.c_void_p(out8.data_ptr()) if srgb else None),
                  "srt_denoise_run_albedo")
        del keep, raw
        return (out, out8) if srgb else out
