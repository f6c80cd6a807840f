"""An independent numpy float32 restatement of the temporal reprojection of include/srt_temporal.h (DESIGN.md
section 5, "Temporal reprojection"), for the tests.  It never calls into the library.

The definition only uses + - * /, min, abs, floor and comparisons in fp32, in source order, so numpy float32
arithmetic reproduces the kernel bit for bit.  `TemporalRef.accumulate` is the vectorised form;
`accumulate(..., naive=True)` is a per-pixel scalar loop of the same definition, used to cross-check the first
on small images.  A guide is denoise_ref.make_guide's dict; a camera is (origin, front, right, up).
"""
from __future__ import annotations

import numpy as np

MISS = 0xFFFFFFFF
F = np.float32
F0, F1, FH = F(0.0), F(1.0), F(0.5)


def camera_vectors(position, yaw, pitch):
    """(origin, front, right, up) as RayTracer::Camera::UpdateCameraVectors builds them from yaw and pitch in
    degrees: front = normalize(cos y cos p, sin p, sin y cos p), right = normalize(cross(front, +Y)),
    up = normalize(cross(right, front)); cos and sin in double, rounded to float32."""
    y, p = np.float64(F(yaw) * F(np.pi / 180.0)), np.float64(F(pitch) * F(np.pi / 180.0))

    def norm(v):
        v = np.asarray(v, F)
        return (v * (F1 / np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2], dtype=F))).astype(F)

    def cross(a, b):
        return np.asarray([a[1] * b[2] - b[1] * a[2], a[2] * b[0] - b[2] * a[0], a[0] * b[1] - b[0] * a[1]], F)

    front = norm([F(np.cos(y)) * F(np.cos(p)), F(np.sin(p)), F(np.sin(y)) * F(np.cos(p))])
    right = norm(cross(front, np.asarray([0, 1, 0], F)))
    up = norm(cross(right, front))
    return np.asarray(position, F), front, right, up


def as_camera(cam):
    if hasattr(cam, "getOrigin"):
        cam = (cam.getOrigin(), cam.getForward(), cam.getRightVector(), cam.getUpVector())
    return tuple(np.asarray(v, F).reshape(3).copy() for v in cam)


def dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def pixel_dirs(cam, W, H):
    """d = (p00 + i*du + j*dv) - o per pixel, (H, W, 3), as srt_denoise_primary_rays computes it."""
    o, f, r, u = as_camera(cam)
    du, dv = r / F(W), u / F(H)
    p00 = (((o + f) - r / F(2)) - u / F(2)) + FH * (du + dv)
    fi = np.arange(W, dtype=F)[None, :, None]
    fj = np.arange(H, dtype=F)[:, None, None]
    return (((p00 + fi * du) + fj * dv) - o).astype(F)


def reproject(t, cam, prev_cam, W, H):
    """Steps 3-5: (a, uu, vv) of every pixel, float32 (H, W), whatever the pixel's guide says."""
    o = as_camera(cam)[0]
    po, pf, pr, pu = as_camera(prev_cam)
    with np.errstate(all="ignore"):
        x = np.asarray(t, F)[..., None] * pixel_dirs(cam, W, H) + o
        v = x - po
        a = dot3(v, pf) / dot3(pf, pf)
        b = dot3(v, pr) / dot3(pr, pr)
        c = dot3(v, pu) / dot3(pu, pu)
        uu = (b / a + FH) * F(W) - FH
        vv = (c / a + FH) * F(H) - FH
    assert a.dtype == F and uu.dtype == F and vv.dtype == F
    return a, uu, vv


def guide_id(g):
    return np.where(g["tri"] == MISS, np.uint32(MISS), g["bvh"]).astype(np.uint32)


class TemporalRef:
    def __init__(self, width, height, max_history=32, depth_tol=0.05, normal_min=0.9):
        self.W, self.H = int(width), int(height)
        self.max_history, self.depth_tol, self.normal_min = F(max_history), F(depth_tol), F(normal_min)
        self.prev = None
        self.frames = 0

    def reset(self):
        self.prev = None
        self.frames = 0

    def accumulate(self, accum, frames, g, cam, naive=False):
        """(H, W, 4) float32: (colour, N).  The result and the guide become the history."""
        C = (np.asarray(accum, F)[..., :3] / F(frames)).astype(F)
        cam = as_camera(cam)
        out = (self._naive if naive else self._vector)(C, g, cam)
        assert out.dtype == F
        self.prev = {"col": out[..., :3].copy(), "N": out[..., 3].copy(), "id": guide_id(g),
                     "normal": np.asarray(g["normal"], F).copy(), "t": np.asarray(g["t"], F).copy(), "cam": cam}
        self.frames += 1
        return out

    # -- the shifted-array form ---------------------------------------------------
    def _vector(self, C, g, cam):
        W, H, P = self.W, self.H, self.prev
        out = np.empty((H, W, 4), F)
        out[..., :3], out[..., 3] = C, F1
        if P is None:
            return out
        idp = guide_id(g)
        n = np.asarray(g["normal"], F)
        a, uu, vv = reproject(g["t"], cam, P["cam"], W, H)
        with np.errstate(all="ignore"):
            ok = (idp != MISS) & (a > 0)
            ok &= (uu >= -1) & (uu < F(W)) & (vv >= -1) & (vv < F(H))
            fu, fv = np.floor(uu), np.floor(vv)
            i0 = np.where(ok, fu, F0).astype(np.int64)
            j0 = np.where(ok, fv, F0).astype(np.int64)
            fx, fy = uu - fu, vv - fv
            sw = np.zeros((H, W), F)
            sm = np.zeros((H, W, 3), F)
            Nh = np.full((H, W), np.inf, F)
            for dy in (0, 1):
                for dx in (0, 1):
                    qx, qy = i0 + dx, j0 + dy
                    inside = (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
                    qx, qy = np.clip(qx, 0, W - 1), np.clip(qy, 0, H - 1)
                    wb = (fx if dx else F1 - fx) * (fy if dy else F1 - fy)
                    nq, tq, cq = P["normal"][qy, qx], P["t"][qy, qx], P["col"][qy, qx]
                    take = ok & inside & (P["id"][qy, qx] == idp)
                    take &= dot3(n, nq) >= self.normal_min
                    take &= np.abs(a - tq) <= self.depth_tol * (a + tq)
                    take &= np.isfinite(cq).all(-1) & (wb > 0)
                    sw = np.where(take, sw + wb, sw)
                    sm = np.where(take[..., None], sm + wb[..., None] * cq, sm)
                    Nh = np.where(take, np.minimum(Nh, P["N"][qy, qx]), Nh)
            has = sw > 0
            hist = sm / sw[..., None]
            Np = np.minimum(Nh + F1, self.max_history)
            k = F1 / Np
            blend = hist + k[..., None] * (C - hist)
            cfin = np.isfinite(C).all(-1)
            out[..., :3] = np.where((has & cfin)[..., None], blend, np.where(has[..., None], hist, C))
            out[..., 3] = np.where(has & cfin, Np, np.where(has, Nh, F1))
        return out

    # -- one pixel and one tap at a time -------------------------------------------
    def _naive(self, C, g, cam):
        W, H, P = self.W, self.H, self.prev
        out = np.empty((H, W, 4), F)
        out[..., :3], out[..., 3] = C, F1
        if P is None:
            return out
        o, f, r, u = cam
        po, pf, pr, pu = P["cam"]
        du, dv = r / F(W), u / F(H)
        p00 = (((o + f) - r / F(2)) - u / F(2)) + FH * (du + dv)
        sdot = lambda a, b: (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]  # noqa: E731
        with np.errstate(all="ignore"):
            for j in range(H):
                for i in range(W):
                    if g["tri"][j, i] == MISS:
                        continue
                    ident, n = g["bvh"][j, i], g["normal"][j, i]
                    d = ((p00 + F(i) * du) + F(j) * dv) - o
                    v = (F(g["t"][j, i]) * d + o) - po
                    a, b, c = sdot(v, pf) / sdot(pf, pf), sdot(v, pr) / sdot(pr, pr), sdot(v, pu) / sdot(pu, pu)
                    if not a > 0:
                        continue
                    uu, vv = (b / a + FH) * F(W) - FH, (c / a + FH) * F(H) - FH
                    if not (uu >= -1 and uu < F(W) and vv >= -1 and vv < F(H)):
                        continue
                    fu, fv = np.floor(uu), np.floor(vv)
                    i0, j0, fx, fy = int(fu), int(fv), uu - fu, vv - fv
                    sw, sm, Nh = F0, [F0, F0, F0], F(np.inf)
                    for dy in (0, 1):
                        for dx in (0, 1):
                            qx, qy = i0 + dx, j0 + dy
                            if not (0 <= qx < W and 0 <= qy < H):
                                continue
                            if P["id"][qy, qx] == MISS or P["id"][qy, qx] != ident:
                                continue
                            if not sdot(n, P["normal"][qy, qx]) >= self.normal_min:
                                continue
                            tq = P["t"][qy, qx]
                            if not np.abs(a - tq) <= self.depth_tol * (a + tq):
                                continue
                            cq = P["col"][qy, qx]
                            if not np.isfinite(cq).all():
                                continue
                            wb = (fx if dx else F1 - fx) * (fy if dy else F1 - fy)
                            if not wb > 0:
                                continue
                            sw = sw + wb
                            sm = [sm[k] + wb * cq[k] for k in range(3)]
                            Nh = min(Nh, P["N"][qy, qx])
                    if not sw > 0:
                        continue
                    hist = [sm[k] / sw for k in range(3)]
                    if np.isfinite(C[j, i]).all():
                        Np = min(Nh + F1, self.max_history)
                        k1 = F1 / Np
                        out[j, i] = [hist[k] + k1 * (C[j, i, k] - hist[k]) for k in range(3)] + [Np]
                    else:
                        out[j, i] = hist + [Nh]
        return out


def two_wall_guide(cam, W, H):
    """The pixel-centre rays of `cam` against two axis-aligned walls, by ray-plane intersection: the front square
    z = 1, |x - 0.3| < 0.4, |y| < 0.4 (BVH record 1) before the back wall z = 0, |x| < 1.5, |y| < 1 (record 0), both
    with normal (0, 0, 1); everything else a miss (t = 1e30, normal 0).  `t` is in units of the unnormalised ray
    direction, as srt_query_closest reports it.  Returns (tri, t, normal, bvh)."""
    o = as_camera(cam)[0]
    d = pixel_dirs(cam, W, H)
    tri = np.full((H, W), MISS, np.uint32)
    t = np.full((H, W), 1e30, F)
    bvh = np.zeros((H, W), np.uint32)
    nrm = np.zeros((H, W, 3), F)
    with np.errstate(all="ignore"):
        for z, rec, inside in ((F(0), 0, lambda x, y: (np.abs(x) < 1.5) & (np.abs(y) < 1.0)),
                               (F(1), 1, lambda x, y: (np.abs(x - F(0.3)) < 0.4) & (np.abs(y) < 0.4))):
            s = (z - o[2]) / d[..., 2]
            x, y = o[0] + s * d[..., 0], o[1] + s * d[..., 1]
            hit = (s > 0) & inside(x, y)
            tri[hit], bvh[hit], t[hit] = 7 + rec, rec, s[hit].astype(F)
            nrm[hit] = (0, 0, 1)
    return tri, t, nrm, bvh
