"""Device-resident batched ray queries (include/srt_query.h): closest hit and occlusion.

``Query(scene)`` uploads a copy of the scene to the device; ``closest(rays)`` and ``occluded(rays)`` trace a
``torch`` tensor of rays that already lives there and return device tensors, without a host round trip or a
synchronisation.  The results are bit-identical to the CPU oracle's ``trace_closest``.  A numpy structured
array of ``RAY_DTYPE`` is accepted too; that path copies both ways and synchronises.  ``sort=True`` on either call
traces the rays in a coherence-sorted order built on the device (include/srt_query_sort.h): the same results.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import RAY_DTYPE, VERT_DTYPE, Scene, _ptr
from ._lib import SRT_QUERY_REFIT, check, lib
from ._stage import _Stage, rays_arg, verts_arg

__all__ = ["Query", "Hits", "HIT_DTYPE", "MISS"]

MISS = 0xFFFFFFFF
# srt_hit, 32 B
HIT_DTYPE = np.dtype([("triangle", "<u4"), ("t", "<f4"), ("normal", "<f4", 3), ("material", "<u4"), ("bvh", "<u4"),
                      ("pad", "<u4")])
assert HIT_DTYPE.itemsize == 32


class Hits:
    """``srt_hit`` records on the device: ``raw`` is the ``[n, 8]`` int32 storage, the properties view its
    fields (no copies).  ``triangle`` is int32, so a miss (0xFFFFFFFF) reads -1; ``hit`` is the boolean mask."""

    def __init__(self, raw):
        self.raw = raw

    def __len__(self):
        return self.raw.shape[0]

    @property
    def triangle(self):
        return self.raw[:, 0]

    @property
    def hit(self):
        return self.raw[:, 0] != -1

    @property
    def t(self):
        import torch
        return self.raw[:, 1].view(torch.float32)

    @property
    def normal(self):
        import torch
        return self.raw[:, 2:5].view(torch.float32)

    @property
    def material(self):
        return self.raw[:, 5]

    @property
    def bvh(self):
        return self.raw[:, 6]

    def numpy(self) -> np.ndarray:
        """The records on the host as a ``HIT_DTYPE`` array (copies and synchronises)."""
        return self.raw.cpu().numpy().view(HIT_DTYPE).reshape(-1)


class Query(_Stage):
    """A ray-query object over ``scene`` (a :class:`srt_amd.Scene`) on ``device``.

    ``stream``: a ``torch.cuda.Stream`` or a raw ``hipStream_t`` handle the queries run on.  With the default
    (None) the object runs on a stream of its own and orders every call with ``torch.cuda.current_stream()``
    by events -- the call waits for the work already queued there, and that stream waits for the results -- so
    it behaves as if it ran on the current stream, whichever that is at the time of the call.

    ``refit=True`` (``SRT_QUERY_REFIT``, include/srt_refit.h) also uploads the vertex indices and a refit
    schedule, so :meth:`refit` can move the object to new vertex positions on the device.  ``rebuild=True`` (with
    ``refit=True``, one model; include/srt_rebuild.h) also allocates what :meth:`rebuild` needs to give the object a
    new tree on the device; ``rebuild_leaf=n`` is :meth:`set_rebuild_leaf` at creation.  ``rebuild_models=True`` (with
    ``refit=True``; include/srt_rebuild_models.h) is ``rebuild=True`` for a scene of any number of models: every BVH
    record gets a new tree over its own triangles.
    """

    _prefix = "srt_query"

    def __init__(self, scene: Scene, device: int = 0, stream=None, refit: bool = False, rebuild: bool = False,
                 rebuild_leaf: int | None = None, rebuild_models: bool = False):
        super().__init__(device, stream)
        if rebuild and not refit:
            raise ValueError("rebuild=True needs refit=True (include/srt_rebuild.h)")
        if rebuild_models and not refit:
            raise ValueError("rebuild_models=True needs refit=True (include/srt_rebuild_models.h)")
        if rebuild and rebuild_models:
            raise ValueError("rebuild=True and rebuild_models=True exclude each other")
        if rebuild_leaf is not None and not (rebuild or rebuild_models):
            raise ValueError("rebuild_leaf needs rebuild=True (include/srt_rebuild_leaf.h)")
        s = scene
        args = (_ptr(s.bvhs), len(s.bvhs), _ptr(s.nodes), len(s.nodes), _ptr(s.tris), len(s.tris), _ptr(s.verts),
                len(s.verts))
        self._n_tris = len(s.tris)
        self._sorted_n = 0  # of the last sort=True call that launched
        if refit:
            self._create(*args, SRT_QUERY_REFIT, name="create_ex")
        else:
            self._create(*args)
        if rebuild or rebuild_models:
            try:
                if rebuild_models:
                    self.enable_rebuild_models()
                else:
                    self.enable_rebuild()
                if rebuild_leaf is not None:
                    self.set_rebuild_leaf(rebuild_leaf)
            except Exception:
                self.close()
                raise

    # -- state ----------------------------------------------------------------
    def set_bvh_count(self, bvh_count: int):
        check(lib().srt_query_set_bvh_count(self.handle, int(bvh_count)), "srt_query_set_bvh_count")

    def update_model_matrix(self, index: int, matrix):
        """``AssetUtils::UpdateModelMatrix``; ``matrix`` is glm column-major (m[c][r])."""
        m = np.ascontiguousarray(np.asarray(matrix, np.float32).reshape(4, 4)).reshape(16)
        check(lib().srt_query_update_model_matrix(self.handle, int(index), _ptr(m)), "srt_query_update_model_matrix")

    # -- refit ----------------------------------------------------------------
    def refit(self, verts):
        """Refit the device scene to new vertices (``srt_query_refit``): a contiguous float32 ``[n_verts, 8]``
        tensor of ``srt_vertex`` records on the object's device -- only enqueued, ordered with the queries as
        ``closest`` is -- or a numpy ``VERT_DTYPE`` array, which is uploaded first and synchronises."""
        import torch
        if isinstance(verts, np.ndarray):
            host = np.ascontiguousarray(verts, dtype=VERT_DTYPE).view(np.float32).reshape(-1, 8)
            self.refit(torch.from_numpy(host).to(f"cuda:{self.device}"))
            self.synchronize()  # the upload may go once the kernels have read it
            return
        if (verts.dtype != torch.float32 or not verts.is_cuda or verts.device.index != self.device
                or not verts.is_contiguous() or verts.dim() != 2 or verts.shape[1] != 8):
            raise ValueError(f"verts must be a contiguous float32 [n_verts, 8] tensor on cuda:{self.device} "
                             "(srt_vertex fields)")
        self._run(lambda: lib().srt_query_refit(self.handle, C.c_void_p(verts.data_ptr()), verts.shape[0]),
                  "srt_query_refit")

    # -- rebuild --------------------------------------------------------------
    def enable_rebuild(self):
        """``srt_query_enable_rebuild``: allocates what :meth:`rebuild` needs (``Query(..., rebuild=True)`` calls it)."""
        check(lib().srt_query_enable_rebuild(self.handle), "srt_query_enable_rebuild")

    def enable_rebuild_models(self):
        """``srt_query_enable_rebuild_models`` (include/srt_rebuild_models.h): :meth:`enable_rebuild` for a scene of any
        number of models (``Query(..., rebuild_models=True)`` calls it).  Every triangle must belong to exactly one BVH
        record."""
        check(lib().srt_query_enable_rebuild_models(self.handle), "srt_query_enable_rebuild_models")

    def set_rebuild_leaf(self, max_leaf: int):
        """``srt_query_set_rebuild_leaf`` (include/srt_rebuild_leaf.h): from the next :meth:`rebuild` on, every subtree
        of the linear BVH that covers at most ``max_leaf`` triangles (1..255; 1, the default, is one triangle a leaf)
        becomes one leaf.  Enqueues nothing."""
        if not 0 <= int(max_leaf) <= 0xFFFFFFFF:
            raise ValueError("max_leaf must be in [1, 255]")
        check(lib().srt_query_set_rebuild_leaf(self.handle, int(max_leaf)), "srt_query_set_rebuild_leaf")

    def rebuild(self, verts):
        """A new tree over the triangles at ``verts`` (``srt_query_rebuild``, include/srt_rebuild.h): a linear BVH
        built on the device.  ``verts`` as :meth:`refit` takes them.  Ordered with the queries as ``closest`` is, but
        not enqueue-only: the call synchronises the object's stream once.  ``Hits.triangle`` keeps meaning the
        scene's triangle index."""
        import torch
        if isinstance(verts, np.ndarray):
            host = np.ascontiguousarray(verts, dtype=VERT_DTYPE).view(np.float32).reshape(-1, 8)
            self.rebuild(torch.from_numpy(host).to(f"cuda:{self.device}"))
            self.synchronize()  # the upload may go once the kernels have read it
            return
        verts_arg(verts, self.device)
        self._run(lambda: lib().srt_query_rebuild(self.handle, C.c_void_p(verts.data_ptr()), verts.shape[0]),
                  "srt_query_rebuild")

    def tri_order(self) -> np.ndarray:
        """Position -> scene triangle index of the device's triangle records (``srt_query_tri_order``: a test and
        debug readback; synchronises).  The identity before any rebuild."""
        out = np.zeros(self._n_tris, np.uint32)
        check(lib().srt_query_tri_order(self.handle, _ptr(out), len(out)), "srt_query_tri_order")
        return out

    def layout(self):
        """The device arrays ``(pairs, roots, tris)`` of csrc/query_host.hpp's layout as uint32 ``[n, 4]`` numpy
        arrays, one 16-B value a row (``srt_query_copy_layout``: a test and debug readback; synchronises)."""
        out = [np.zeros((self.get_int("layout." + name) // 16, 4), np.uint32) for name in ("pairs", "roots", "tris")]
        check(lib().srt_query_copy_layout(self.handle, *[_ptr(a) for a in out]), "srt_query_copy_layout")
        return tuple(out)

    # -- queries --------------------------------------------------------------
    def _trace(self, fn, what, rays, out):
        self._run(lambda: fn(self.handle, C.c_void_p(rays.data_ptr()), rays.shape[0], C.c_void_p(out.data_ptr())), what)
        return out

    def closest(self, rays, sort=False):
        """Closest hits of ``rays``: a :class:`Hits` over a device tensor (torch input), or a ``HIT_DTYPE``
        array (numpy ``RAY_DTYPE`` input).  ``sort=True`` traces the rays in a coherence-sorted order built on the
        device (``srt_query_closest_sorted``, include/srt_query_sort.h): the same results bit for bit, faster for rays
        that arrive incoherent and slower for rays that arrive coherent."""
        import torch
        if isinstance(rays, np.ndarray):
            dev = torch.from_numpy(np.ascontiguousarray(rays, dtype=RAY_DTYPE).view(np.float32).reshape(-1, 8))
            hits = self.closest(dev.to(f"cuda:{self.device}"), sort=sort)
            self.synchronize()
            return hits.numpy()
        rays_arg(rays, self.device)
        out = torch.empty((rays.shape[0], 8), dtype=torch.int32, device=rays.device)
        if sort:
            self._sorted_n = rays.shape[0] or self._sorted_n
            return Hits(self._trace(lib().srt_query_closest_sorted, "srt_query_closest_sorted", rays, out))
        return Hits(self._trace(lib().srt_query_closest, "srt_query_closest", rays, out))

    def occluded(self, rays, sort=False):
        """1 where some triangle is accepted (the walk stops at the first): a uint8 ``[n]`` device tensor, or
        a numpy array for numpy input.  ``sort=True``: ``srt_query_occluded_sorted``, as :meth:`closest`."""
        import torch
        if isinstance(rays, np.ndarray):
            dev = torch.from_numpy(np.ascontiguousarray(rays, dtype=RAY_DTYPE).view(np.float32).reshape(-1, 8))
            occ = self.occluded(dev.to(f"cuda:{self.device}"), sort=sort)
            self.synchronize()
            return occ.cpu().numpy()
        rays_arg(rays, self.device)
        out = torch.empty((rays.shape[0],), dtype=torch.uint8, device=rays.device)
        if sort:
            self._sorted_n = rays.shape[0] or self._sorted_n
            return self._trace(lib().srt_query_occluded_sorted, "srt_query_occluded_sorted", rays, out)
        return self._trace(lib().srt_query_occluded, "srt_query_occluded", rays, out)

    def ray_order(self):
        """``(order, keys)`` of the last ``sort=True`` call (``srt_query_copy_ray_order``: a test and debug readback;
        synchronises): position -> ray index, and the sorted keys.  ``SrtError`` (``SRT_ERR_STATE``) before any."""
        n = self._sorted_n
        order, keys = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        check(lib().srt_query_copy_ray_order(self.handle, _ptr(order), _ptr(keys), n), "srt_query_copy_ray_order")
        return order, keys

