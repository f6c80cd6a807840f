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
from ._stage import _Stage, accum_arg, get_params, hits_arg, updated_params, verts_arg

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


class Temporal(_Stage):
    """A temporal accumulator for ``width`` x ``height`` frames on ``device``.

    ``stream``: a ``torch.cuda.Stream`` or a raw ``hipStream_t`` handle.  With the default (None) the object runs
    on a stream of its own and orders every call with ``torch.cuda.current_stream()`` by events, exactly as
    :class:`srt_amd.denoise.Denoiser` does.
    """

    _prefix = "srt_temporal"

    def __init__(self, width: int, height: int, device: int = 0, stream=None):
        super().__init__(device, stream)
        self._verts = None  # the tensor set_vertices was given
        self.width, self.height = int(width), int(height)
        self._create(self.width, self.height)

    # -- state ----------------------------------------------------------------
    @property
    def params(self) -> dict:
        return get_params(TemporalParams, lib().srt_temporal_get_params, self.handle, "srt_temporal_get_params")

    def set_params(self, **kw):
        """Any of max_history, depth_tol, normal_min; the others keep their values."""
        p = updated_params(TemporalParams, self.params, kw, "temporal")
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

    def set_mesh(self, scene_or_tris, n_verts=None):
        """Attach the mesh whose vertices move (include/srt_temporal_deform.h): a :class:`srt_amd.Scene` (its
        triangles and vertex count), or the ``TRI_DTYPE`` triangle array with ``n_verts``.  ``None`` or an empty
        array detaches it.  Allocates (the vertex indices and the previous positions) and waits for the stream."""
        from . import TRI_DTYPE, _ptr
        if scene_or_tris is None:
            tris, n_verts = np.zeros(0, TRI_DTYPE), 0
        elif hasattr(scene_or_tris, "tris"):
            tris = scene_or_tris.tris
            n_verts = len(scene_or_tris.verts) if n_verts is None else n_verts
        else:
            tris = scene_or_tris
            if n_verts is None:
                raise ValueError("set_mesh: n_verts is needed with a triangle array")
        tris = np.ascontiguousarray(tris, dtype=TRI_DTYPE)
        self._verts = None
        check(lib().srt_temporal_set_mesh(self.handle, _ptr(tris) if len(tris) else None, len(tris), int(n_verts)),
              "srt_temporal_set_mesh")

    def set_vertices(self, verts):
        """The vertices of the frame about to be accumulated: the contiguous float32 ``[n_verts, 8]`` device tensor
        ``Query.refit`` was given.  It is kept alive, and applies to every ``accumulate`` until set again; ``None``
        makes every pixel rigid and drops the previous positions.  Enqueues nothing: the accumulate that reads the
        array is ordered with ``torch.cuda.current_stream()`` as every call is."""
        if verts is None:
            check(lib().srt_temporal_set_vertices(self.handle, None, self.get_int("mesh.verts")), "srt_temporal_set_vertices")
            self._verts = None
            return
        ptr, keep = verts_arg(verts, self.device)
        check(lib().srt_temporal_set_vertices(self.handle, C.c_void_p(ptr), verts.shape[0]), "srt_temporal_set_vertices")
        self._verts = keep

    # -- work -----------------------------------------------------------------
    def accumulate(self, accum, frames: int, hits, camera):
        """Blend the accumulation image ``accum`` (the SUM over ``frames``: a contiguous float32 ``[H, W, 4]``
        device tensor, or a raw device pointer) into the history.  ``hits``: the guide of ``camera``'s pixel-centre
        rays, a :class:`srt_amd.query.Hits` or its ``[W * H, 8]`` int32 tensor.  Returns the float32 ``[H, W, 4]``
        result ``(colour, N)`` on the device."""
        import torch
        dev = f"cuda:{self.device}"
        acc_ptr, keep = accum_arg(accum, self.width, self.height, self.device)
        _, raw = hits_arg(hits, self.width * self.height, self.device)
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
        acc_ptr, keep = accum_arg(accum, self.width, self.height, self.device)
        _, raw = hits_arg(hits, self.width * self.height, self.device)
        cam = _camera(camera)
        out = torch.empty((self.height, self.width, 4), dtype=torch.float32, device=dev)
        mom = torch.empty((self.height, self.width, 4), dtype=torch.float32, device=dev)
        self._run(lambda: lib().srt_temporal_accumulate_moments(self.handle, C.c_void_p(acc_ptr), int(frames),
                                                                C.c_void_p(raw.data_ptr()), C.byref(cam),
                                                                C.c_void_p(out.data_ptr()), C.c_void_p(mom.data_ptr())),
                  "srt_temporal_accumulate_moments")
        del keep
        return out, mom
