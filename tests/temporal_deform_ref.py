"""An independent numpy float32 restatement of the deforming-mesh extension of the temporal reprojection
(include/srt_temporal_deform.h; DESIGN.md section 5, "Deforming meshes"), for the tests.  It never calls into the
library.  `TemporalDeformRef` is variance_ref's object (temporal_motion_ref's with the moment history), with the
attached mesh, V and V' and the RIGID / DEFORMING rule; both `accumulate` and `accumulate_moments` go through the
one `_points` it replaces.  The vectorised form only (`naive` is refused while a mesh is attached).

`grid_scene` and `waved` make the sequence the tests share: refit_ref.grid_triangles(4) (32 triangles) as record 0,
waved with a phase that advances per frame, and a static quad as record 1, seen by temporal_motion_ref's CAMERAS[1:5].
"""
from __future__ import annotations

import numpy as np

import temporal_motion_ref as M
import variance_ref as V
from temporal_ref import F, MISS, dot3, guide_id, pixel_dirs


def affine(m16, x):
    """((M(i,0)*x + M(i,1)*y) + M(i,2)*z) + M(i,3) per row of a column-major matrix, on (..., 3) float32."""
    m = np.asarray(m16, F)
    return np.stack([((m[i] * x[..., 0] + m[4 + i] * x[..., 1]) + m[8 + i] * x[..., 2]) + m[12 + i] for i in range(3)],
                    -1).astype(F)


class TemporalDeformRef(V.VarianceTemporalRef):
    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.tris = None      # (n_tris, 3) vertex indices
        self.n_verts = 0
        self.V = None         # (n_verts, 3) float32: the positions set now
        self.Vp = None        # those the previous accumulate read
        self.deforming = None  # (H, W) bool: the pixels of the last accumulate that took the DEFORMING path

    def set_mesh(self, tris, n_verts):
        tris = np.asarray(tris)
        tris = tris["v"] if tris.dtype.names else tris
        self.tris = None if len(tris) == 0 else tris.reshape(-1, 3).astype(np.int64)
        self.n_verts = int(n_verts) if self.tris is not None else 0
        self.V = self.Vp = None

    def set_vertices(self, verts):
        if verts is None:
            self.V = self.Vp = None
            return
        verts = np.asarray(verts)
        pos = verts["pos"] if verts.dtype.names else verts
        assert self.tris is not None and len(pos) == self.n_verts
        self.V = np.asarray(pos, F).reshape(-1, 3).copy()

    def reset(self):
        super().reset()
        self.Vp = None

    def runs_deform(self):
        return self.tris is not None and self.V is not None

    def _after(self):
        if self.runs_deform():
            self.Vp = self.V.copy()

    def accumulate(self, accum, frames, g, cam, naive=False):
        assert not (naive and self.tris is not None)
        self.deforming = np.zeros((self.H, self.W), bool)  # (_points is not reached without a history)
        out = super().accumulate(accum, frames, g, cam, naive)
        self._after()
        return out

    def accumulate_moments(self, accum, frames, g, cam, naive=False):
        assert not (naive and self.tris is not None)
        self.deforming = np.zeros((self.H, self.W), bool)
        out = super().accumulate_moments(accum, frames, g, cam, naive)  # (it calls TemporalMotionRef.accumulate, not ours)
        self._after()
        return out

    def _corners(self, arr, idx):
        """Positions through indices; an index >= n_verts reads (0, 0, 0)."""
        padded = np.concatenate([arr, np.zeros((1, 3), F)])
        return padded[np.where(idx < self.n_verts, idx, self.n_verts)]

    def _points(self, g, cam):
        x_rigid = super()._points(g, cam)
        self.deforming = np.zeros((self.H, self.W), bool)
        if self.prev is None or not self.runs_deform() or self.Vp is None:
            return x_rigid
        idp = guide_id(g)
        k = np.asarray(g["tri"]).astype(np.int64)
        hit = idp != MISS
        in_mesh = hit & (k < len(self.tris))
        idx = self.tris[np.where(in_mesh, k, 0)]           # (H, W, 3)
        p = [self._corners(self.V, idx[..., c]) for c in range(3)]
        q = [self._corners(self.Vp, idx[..., c]) for c in range(3)]
        same = np.ones((self.H, self.W), bool)
        for a, b in zip(p, q):
            same &= (a.view(np.uint32) == b.view(np.uint32)).all(-1)
        deforming = in_mesh & ~same
        nQ, nP = len(self.Q), len(self.P)
        with np.errstate(all="ignore"):
            x = (np.asarray(g["t"], F)[..., None] * pixel_dirs(cam, self.W, self.H) + cam[0]).astype(F)
            xm = x.copy()
            for r in range(nQ):
                sel = deforming & (idp == r)
                if sel.any():
                    xm[sel] = affine(self.Q[r][0], x[sel])
            e1, e2, v0p = p[1] - p[0], p[2] - p[0], xm - p[0]
            d00, d01, d11, d20, d21 = dot3(e1, e1), dot3(e1, e2), dot3(e2, e2), dot3(v0p, e1), dot3(v0p, e2)
            denom = F(1.0) / (d00 * d11 - d01 * d01)
            v = (d11 * d20 - d01 * d21) * denom
            w = (d00 * d21 - d01 * d20) * denom
            u = (F(1.0) - v) - w
            ym = ((u[..., None] * q[0] + v[..., None] * q[1]) + w[..., None] * q[2]).astype(F)
            xp = ym.copy()
            for r in range(nQ):
                sel = deforming & (idp == r)
                if sel.any():
                    A = self.P[r][1] if r < nP else self.Q[r][1]
                    xp[sel] = affine(A, ym[sel])
        assert xp.dtype == F
        self.deforming = deforming
        return np.where(deforming[..., None], xp, x_rigid)


# ---------------------------------------------------------------------------------------------------------------
# the shared sequence
# ---------------------------------------------------------------------------------------------------------------
W, H, FRAMES = 37, 23, 4
AMPLITUDE, PHASE_STEP = 0.25, 0.6  # tests/test_temporal_deform_ref.py shows the sequence is not vacuous at these
GRID_SCALE, GRID_SHIFT = 0.6, (-1.9, -1.2, 0.0)   # where the 4 x 4 grid over [0, 4]^2 stands in the cameras' view
QUAD = np.asarray([[0.8, -0.8, 0.2, 1.7, -0.8, 0.2, 1.7, 0.8, 0.2], [0.8, -0.8, 0.2, 1.7, 0.8, 0.2, 0.8, 0.8, 0.2]], F)
N_GRID = 32  # triangles of record 0


def grid_scene():
    """(scene, ids): record 0 the bumpy grid, record 1 the quad; `ids` are the grid's vertex indices."""
    import refit_ref as RR
    import srt_amd as S

    grid = (RR.grid_triangles(n=4).reshape(-1, 3, 3) * F(GRID_SCALE) + np.asarray(GRID_SHIFT, F)).astype(F).reshape(-1, 9)
    scene = S.Scene.from_models([S.model_from_triangles(grid), S.model_from_triangles(QUAD)])
    assert len(scene.tris) == N_GRID + 2 and len(scene.bvhs) == 2
    ids = np.unique(scene.tris["v"][:N_GRID])
    assert not np.intersect1d(ids, scene.tris["v"][N_GRID:]).size  # the quad shares no vertex with the grid
    return scene, ids


def waved(scene, ids, k, amplitude=AMPLITUDE, step=PHASE_STEP):
    """The scene's vertices at frame k: the grid's displaced by refit_ref.wave at phase k * step, the quad's as built."""
    import refit_ref as RR

    verts = scene.verts.copy()
    verts["pos"][ids] = RR.wave(scene.verts, amplitude, step * k)["pos"][ids]
    return verts


def pixel_rays(cam, w=W, h=H):
    """RAY_DTYPE pixel-centre rays of `cam`, index j * W + i (denoise_ref.camera_rays)."""
    import denoise_ref as D
    import srt_amd as S

    o, d = D.camera_rays(*cam, w, h)
    rays = np.zeros(w * h, S.RAY_DTYPE)
    rays["o"], rays["d"], rays["t"] = o, d, F(1e30)
    return rays


def oracle_guide(scene, verts, cam, w=W, h=H):
    """The oracle's closest hits of the pixel-centre rays on the host-refit scene, as a guide with the hit's record."""
    import denoise_ref as D
    import srt_amd as S
    from oracle import pyoracle as O

    tri, t, nrm, _ = O.Oracle(S.refit_scene(scene, verts)).trace_closest(len(scene.bvhs), pixel_rays(cam, w, h))
    bvh = np.where(tri == MISS, 0, tri >= N_GRID).astype(np.uint32)
    return D.make_guide(tri.reshape(h, w), t.reshape(h, w), nrm.reshape(h, w, 3), bvh.reshape(h, w))


def hit_barycentrics(g, verts, tris, cam):
    """(v, w) of every hit's point o + t * d in its triangle at `verts`, float64 (for the tests' colour pattern)."""
    h, w = g["tri"].shape
    x = (g["t"][..., None].astype(np.float64) * pixel_dirs(cam, w, h) + cam[0]).astype(np.float64)
    k = np.where(g["tri"] == MISS, 0, g["tri"]).astype(np.int64)
    p = verts["pos"][tris["v"][k]].astype(np.float64)  # (H, W, 3, 3)
    e1, e2, v0p = p[..., 1, :] - p[..., 0, :], p[..., 2, :] - p[..., 0, :], x - p[..., 0, :]
    d00, d01, d11 = (e1 * e1).sum(-1), (e1 * e2).sum(-1), (e2 * e2).sum(-1)
    d20, d21 = (v0p * e1).sum(-1), (v0p * e2).sum(-1)
    den = d00 * d11 - d01 * d01
    return (d11 * d20 - d01 * d21) / den, (d00 * d21 - d01 * d20) / den


def material_pattern(tri, bary_v, bary_w):
    """A noise-free colour fixed to the material: a function of the triangle index and the barycentrics."""
    tri = np.asarray(tri).astype(np.int64)
    base = np.stack([(tri * 37 % 11) / 11.0, (tri * 53 % 7) / 7.0, (tri * 29 % 13) / 13.0], -1)
    ramp = np.stack([bary_v, bary_w, 1.0 - bary_v - bary_w], -1)
    return (0.25 + base + 2.0 * ramp).astype(F)


def sequence_cameras():
    import temporal_ref as T

    return [T.camera_vectors(*c) for c in M.CAMERAS[1:1 + FRAMES]]
