"""Surface attributes of query hits (include/srt_surface.h): albedo, barycentrics and uv.

``Surface(scene)`` uploads what ``TriangleToSupportedMat`` reads -- frames, triangles with their uvs, materials
and, when the scene samples them, its textures -- to the device; ``shade(rays, hits)`` turns the ``srt_hit``
records ``Query.closest`` wrote for ``rays`` into one ``srt_surface_attr`` per ray, on the device, without a host
round trip or a synchronisation.  ``Denoiser.run_albedo`` takes the result.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import Scene, _ptr
from . import _lib
from ._lib import check, lib
from ._lib import SRT_SURFACE_REFIT
from ._stage import _Stage, hits_arg, rays_arg, verts_arg

__all__ = ["Surface", "ATTR_DTYPE"]

# srt_surface_attr, 32 B
ATTR_DTYPE = np.dtype([("albedo", "<f4", 3), ("bary_v", "<f4"), ("bary_w", "<f4"), ("uv", "<f4", 2), ("hit", "<u4")])
assert ATTR_DTYPE.itemsize == 32


def _descs(textures):
    keep = [np.ascontiguousarray(t if t.ndim == 3 else t[:, :, None], np.uint8) for t in textures]
    descs = (_lib.Texture * max(len(keep), 1))(*[_lib.Texture(t.ctypes.data, t.shape[1], t.shape[0], t.shape[2])
                                                  for t in keep])
    return keep, descs


class Surface(_Stage):
    """A surface-attribute object over ``scene`` (a :class:`srt_amd.Scene`) on ``device``.

    As ``Compute.bind_scene`` does, a scene with ``sample_textures`` uploads its textures and passes no
    ``tex_albedo``; otherwise use_texture materials take the constant ``scene.tex_albedo``.  ``stream``: a
    ``torch.cuda.Stream`` or a raw ``hipStream_t`` handle; with the default (None) the object runs on a stream of
    its own and orders every call with ``torch.cuda.current_stream()`` by events, as :class:`srt_amd.query.Query`.
    """

    _prefix = "srt_surface"

    def __init__(self, scene: Scene, device: int = 0, stream=None, refit: bool = False):
        super().__init__(device, stream)
        s = scene
        tex = None if s.sample_textures else np.ascontiguousarray(s.tex_albedo, np.float32)
        args = (_ptr(s.bvhs), len(s.bvhs), _ptr(s.mats), _ptr(tex), len(s.mats), _ptr(s.tris), len(s.tris),
                _ptr(s.verts), len(s.verts))
        if refit:
            self._create(*args, SRT_SURFACE_REFIT, name="create_ex")
        else:
            self._create(*args)
        if s.sample_textures:
            self.upload_textures(s.textures)

    # -- state ----------------------------------------------------------------
    def upload_textures(self, textures):
        """``(H, W, C)`` uint8 arrays, rows top first: texture i gets handle i; replaces any previous set."""
        keep, descs = _descs(textures)
        check(lib().srt_surface_upload_textures(self.handle, descs, len(keep)), "srt_surface_upload_textures")

    def set_bvh_count(self, bvh_count: int):
        check(lib().srt_surface_set_bvh_count(self.handle, int(bvh_count)), "srt_surface_set_bvh_count")

    def update_model_matrix(self, index: int, matrix):
        """``AssetUtils::UpdateModelMatrix``; ``matrix`` is glm column-major (m[c][r])."""
        m = np.ascontiguousarray(np.asarray(matrix, np.float32).reshape(4, 4)).reshape(16)
        check(lib().srt_surface_update_model_matrix(self.handle, int(index), _ptr(m)), "srt_surface_update_model_matrix")

    def refit(self, verts):
        """Move the object's triangles to new vertices (``srt_surface_refit``, include/srt_surface_refit.h): the
        contiguous float32 ``[n_verts, 8]`` device tensor of ``srt_vertex`` records ``Query.refit`` takes -- only
        enqueued, ordered with ``shade`` -- or a numpy ``VERT_DTYPE`` array, which is uploaded first and
        synchronises.  Needs ``Surface(scene, refit=True)``."""
        import torch
        if isinstance(verts, np.ndarray):
            from . import VERT_DTYPE
            host = np.ascontiguousarray(verts, dtype=VERT_DTYPE).view(np.float32).reshape(-1, 8)
            self.refit(torch.from_numpy(host).to(f"cuda:{self.device}"))
            self.synchronize()  # the upload may go once the kernel has read it
            return
        ptr, _ = verts_arg(verts, self.device)
        self._run(lambda: lib().srt_surface_refit(self.handle, C.c_void_p(ptr), verts.shape[0]), "srt_surface_refit")

    # -- work -----------------------------------------------------------------
    def shade(self, rays, hits):
        """``rays``: the contiguous float32 ``[n, 8]`` device tensor of ``srt_ray`` records that was traced;
        ``hits``: its :class:`srt_amd.query.Hits` (or their ``[n, 8]`` int32 tensor).  Returns a float32 ``[n, 8]``
        device tensor of ``srt_surface_attr`` records: columns 0-2 albedo, 3 bary_v, 4 bary_w, 5-6 uv, 7 the hit
        flag as bits (``.cpu().numpy().view(ATTR_DTYPE)`` names them)."""
        import torch
        rays_arg(rays, self.device)
        _, raw = hits_arg(hits, rays.shape[0], self.device, text="hits must be the [n, 8] int32 srt_hit tensor of the rays")
        out = torch.empty((rays.shape[0], 8), dtype=torch.float32, device=rays.device)
        self._run(lambda: lib().srt_surface_shade(self.handle, C.c_void_p(rays.data_ptr()), C.c_void_p(raw.data_ptr()),
                                                  rays.shape[0], C.c_void_p(out.data_ptr())), "srt_surface_shade")
        return out
