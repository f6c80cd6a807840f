"""Temporal reprojection for progressive frames while the camera moves (include/srt_temporal.h).

``Temporal(width, height)`` allocates its history once.  ``accumulate(accum, frames, hits, camera)`` blends the
new frame (a torch tensor, or the raw device pointer ``Compute.image_pointers()`` returns) into the previous
result wherever the same surface point was visible before, and returns ``(colour, N)`` per pixel on the device;
``hits`` is the guide of the pixel-centre rays of ``camera`` (``Denoiser.primary_rays`` + ``Query.closest``).
``Denoiser.run(out, 1, hits)`` filters the result.  Nothing leaves the device and no call synchronises.  Full
frames only.  A model that moves (``UpdateModelMatrix``) is followed when ``set_models`` states the records'
frames each frame (include/srt_temporal_motion.h); without it, call ``reset()`` after a model-matrix change, and
after a scene change in any case.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import TemporalCamera, TemporalModel, TemporalParams, check, lib

__all__ = ["Temporal"]


def _camera(camera) -> TemporalCamera:
    """An srt_temporal_camera from a camera object (getOrigin / getForward / getRightVector / getUpVector) or a
    sequence (origin, front, right, up)."""
    if hasattr(camera, "getOrigin"):
        camera = (camera.getOrigin(), camera.getForward(), camera.getRightVector(), camera.getUpVector())
    vec = [np.asarray(v, np.float32).reshape(3) for v in camera]
    if len(vec) != 4:
        raise ValueError("camera: an object with getOrigin/getForward/getRightVector/getUpVector or 4 vectors")
    return TemporalCamera(*[(C.c_float * 3)(*[float(x) for x in v]) for v in vec])


class Temporal:
    """A temporal accumulator for ``width`` x ``height`` frames on ``device``.

    ``stream``: a ``torch.cuda.Stream`` or a raw ``hipStream_t`` handle.  With the default (None) the object runs
    on a stream of its own and orders every call with ``torch.cuda.current_stream()`` by events, exactly as
    :class:`srt_amd.denoise.Denoiser` does.
    """

    def __init__(self, width: int, height: int, device: int = 0, stream=None):
        self.width, self.height, self.device = int(width), int(height), int(device)
        self._d = None
        self._ext = None
        handle = getattr(stream, "cuda_stream", stream)
        self._own_stream = not handle
        h = C.c_void_p()
        check(lib().srt_temporal_create(self.device, C.c_void_p(handle) if handle else None, self.width, self.height,
                                        C.byref(h)), "srt_temporal_create")
        self._d = h

    # -- lifecycle ------------------------------------------------------------
    def close(self):
        if self._d is not None:
            lib().srt_temporal_destroy(self._d)
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
            raise RuntimeError("Temporal is closed")
        return self._d

    # -- state ----------------------------------------------------------------
    def get_int(self, name: str) -> int:
        v = C.c_int()
        check(lib().srt_temporal_get_int(self.handle, name.encode(), C.byref(v)), f"srt_temporal_get_int({name})")
        return v.value

    @property
    def params(self) -> dict:
        p = TemporalParams()
        check(lib().srt_temporal_get_params(self.handle, C.byref(p)), "srt_temporal_get_params")
        return {n: getattr(p, n) for n, _ in TemporalParams._fields_}

    def set_params(self, **kw):
        """Any of max_history, depth_tol, normal_min; the others keep their values."""
        cur = self.params
        unknown = set(kw) - set(cur)
        if unknown:
            raise TypeError(f"unknown temporal parameter(s): {sorted(unknown)}")
        cur.update(kw)
        mh = int(cur["max_history"])
        if not 0 <= mh <= 0xFFFFFFFF:
            raise ValueError("max_history must fit an unsigned 32-bit integer")
        p = TemporalParams(mh, float(cur["depth_tol"]), float(cur["normal_min"]))
        check(lib().srt_temporal_set_params(self.handle, C.byref(p)), "srt_temporal_set_params")

    def reset(self):
        """Drop the history: the next ``accumulate`` behaves as the first."""
        check(lib().srt_temporal_reset(self.handle), "srt_temporal_reset")

    def set_models(self, frames, models=None):
        """State the pose of BVH records ``0..n-1`` for the frames accumulated from now on (it persists until set
        again; an empty ``frames`` returns to the static behaviour).  ``frames``: ``[n, 16]`` or ``[n, 4, 4]``
        float32, each the record's ``frame`` (world -> model) as ``UpdateModelMatrix`` takes it, glm column-major
        (m[c][r]).  ``models``: the inverses (model -> world) in the same layout; when omitted each is computed in
        float64 by ``srt_temporal_model_from_frame``."""
        f = np.ascontiguousarray(np.asarray(frames, np.float32).reshape(-1, 16))
        n = len(f)
        arr = (TemporalModel * max(n, 1))()
        if models is None:
            for k in range(n):
                check(lib().srt_temporal_model_from_frame(f[k].ctypes.data_as(C.c_void_p), C.byref(arr[k])),
                      f"srt_temporal_model_from_frame(record {k})")
        else:
            m = np.ascontiguousarray(np.asarray(models, np.float32).reshape(-1, 16))
            if len(m) != n:
                raise ValueError("models: one model_to_world per frame")
            both = np.ascontiguousarray(np.concatenate([f, m], axis=1))
            C.memmove(arr, both.ctypes.data, both.nbytes)
        check(lib().srt_temporal_set_models(self.handle, arr, n), "srt_temporal_set_models")

    # -- work -----------------------------------------------------------------
    def _ordered(self, torch):
        if not self._own_stream:
            return None
        if self._ext is None:
            self._ext = torch.cuda.ExternalStream(int(lib().srt_temporal_stream(self.handle)), device=self.device)
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

    def accumulate(self, accum, frames: int, hits, camera):
        """Blend the accumulation image ``accum`` (the SUM over ``frames``: a contiguous float32 ``[H, W, 4]``
        device tensor, or a raw device pointer) into the history.  ``hits``: the guide of ``camera``'s pixel-centre
        rays, a :class:`srt_amd.query.Hits` or its ``[W * H, 8]`` int32 tensor.  Returns the float32 ``[H, W, 4]``
        result ``(colour, N)`` on the device."""
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
        if raw is None or (raw.dtype != torch.int32 or not raw.is_cuda or raw.device.index != self.device
                           or not raw.is_contiguous() or tuple(raw.shape) != (self.width * self.height, 8)):
            raise ValueError(f"hits must be the [W * H, 8] int32 srt_hit tensor on {dev}")
        cam = _camera(camera)
        out = torch.empty((self.height, self.width, 4), dtype=torch.float32, device=dev)
        self._run(lambda: lib().srt_temporal_accumulate(self.handle, C.c_void_p(acc_ptr), int(frames),
                                                        C.c_void_p(raw.data_ptr()), C.byref(cam),
                                                        C.c_void_p(out.data_ptr())), "srt_temporal_accumulate")
        del keep
        return out

    def enable_moments(self):
        """Allocate the luminance-moment history (include/srt_variance.h); idempotent."""
        check(lib().srt_temporal_enable_moments(self.handle), "srt_temporal_enable_moments")

    def accumulate_moments(self, accum, frames: int, hits, camera):
        """``accumulate``, and the per-pixel luminance moments: returns ``(out, moments)``, ``out`` bit for bit what
        ``accumulate`` returns and ``moments`` a float32 ``[H, W, 4]`` device tensor ``(m1, m2, variance, N)`` for
        ``Denoiser.run_variance``.  Needs ``enable_moments()``."""
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
        if raw is None or (raw.dtype != torch.int32 or not raw.is_cuda or raw.device.index != self.device
                           or not raw.is_contiguous() or tuple(raw.shape) != (self.width * self.height, 8)):
            raise ValueError(f"hits must be the [W * H, 8] int32 srt_hit tensor on {dev}")
        cam = _camera(camera)
        out = torch.empty((self.height, self.width, 4), dtype=torch.float32, device=dev)
        mom = torch.empty((self.height, self.width, 4), dtype=torch.float32, device=dev)
        self._run(lambda: lib().srt_temporal_accumulate_moments(self.handle, C.c_void_p(acc_ptr), int(frames),
                                                                C.c_void_p(raw.data_ptr()), C.byref(cam),
                                                                C.c_void_p(out.data_ptr()), C.c_void_p(mom.data_ptr())),
                  "srt_temporal_accumulate_moments")
        del keep
        return out, mom

    def synchronize(self):
        """Wait for the work enqueued so far."""
        import torch
        torch.cuda.ExternalStream(int(lib().srt_temporal_stream(self.handle) or 0), device=self.device).synchronize()
