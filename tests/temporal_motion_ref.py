"""An independent numpy float32 restatement of the moving-model extension of the temporal reprojection
(include/srt_temporal_motion.h; DESIGN.md section 5, "Moving models"), for the tests.  It never calls into the
library.  It imports temporal_ref and adds the pose bookkeeping (P, Q, STATIC / MOVING), the 3 x 4 product M_r
and a variant of the two-wall guide whose records are posed by matrices.

A pose is (world_to_model, model_to_world), each 16 float32 in glm column-major order: element (row i, column k)
is m[4 * k + i].  `TemporalMotionRef.accumulate` is the vectorised form; `naive=True` is a per-pixel scalar loop
of the same definition.
"""
from __future__ import annotations

import numpy as np

import temporal_ref as T
from temporal_ref import F, F0, F1, FH, MISS, as_camera, dot3, guide_id, pixel_dirs

IDENTITY = np.eye(4, dtype=F).reshape(16)


def pose_from_frame(frame):
    """(frame, inverse) with the inverse by numpy in float64, its bottom row set to (0, 0, 0, 1), rounded to
    float32.  reshape(4, 4) of a column-major matrix is its transpose, and inverting commutes with transposing."""
    frame = np.asarray(frame, F).reshape(16)
    inv = np.linalg.inv(frame.astype(np.float64).reshape(4, 4))
    inv[:, 3] = (0, 0, 0, 1)
    return frame.copy(), inv.reshape(16).astype(F)


def pose_from_model(model_to_world):
    m2w, w2m = pose_from_frame(model_to_world)
    return w2m, m2w


def column_major(rows3x3=np.eye(3), translation=(0, 0, 0)):
    """The 16 floats of the affine matrix with the given 3 x 3 part (row-major, as written on paper) and translation."""
    m = np.eye(4)
    m[:3, :3] = rows3x3
    m[:3, 3] = translation
    return m.T.reshape(16).astype(F)


def rotation(axis, degrees):
    c, s = np.cos(np.radians(degrees)), np.sin(np.radians(degrees))
    k = "xyz".index(axis)
    r = np.eye(3)
    a, b = (k + 1) % 3, (k + 2) % 3
    r[a, a], r[a, b], r[b, a], r[b, b] = c, -s, s, c
    return r


def compose(prev_pose, cur_pose):
    """M = prev.model_to_world o cur.world_to_model as 3 rows of 4, float32:
    M(i, j) = (A(i,0)*B(0,j) + A(i,1)*B(1,j)) + A(i,2)*B(2,j), and + A(i,3) for j == 3."""
    a, b = np.asarray(prev_pose[1], F), np.asarray(cur_pose[0], F)
    m = np.empty((3, 4), F)
    for i in range(3):
        for j in range(4):
            e = (a[i] * b[4 * j] + a[4 + i] * b[4 * j + 1]) + a[8 + i] * b[4 * j + 2]
            m[i, j] = e + a[12 + i] if j == 3 else e
    return m


def xform(m16, v, w):
    """traversal.hpp's xform: ((m0*x + m4*y) + m8*z) + m12*w per row, on (..., 3) float32."""
    m = np.asarray(m16, F)
    v = np.asarray(v, F)
    return np.stack([((m[i] * v[..., 0] + m[4 + i] * v[..., 1]) + m[8 + i] * v[..., 2]) + m[12 + i] * F(w)
                     for i in range(3)], -1).astype(F)


def same_pose(p, q):
    return all(np.array_equal(np.asarray(a, F).view(np.uint32), np.asarray(b, F).view(np.uint32)) for a, b in zip(p, q))


class TemporalMotionRef(T.TemporalRef):
    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.Q = []   # the current poses
        self.P = []   # those of the previous accumulated frame

    def set_models(self, poses):
        self.Q = [(np.asarray(w, F).reshape(16).copy(), np.asarray(m, F).reshape(16).copy()) for w, m in poses]

    def reset(self):
        super().reset()
        self.P = []

    def motion(self):
        """(moving [n_Q] bool, M [n_Q, 3, 4] float32) for the frame about to be accumulated."""
        n = len(self.Q)
        moving = np.zeros(n, bool)
        M = np.zeros((n, 3, 4), F)
        M[:, :, :3] = np.eye(3, dtype=F)
        for r in range(min(len(self.P), n)):
            if not same_pose(self.P[r], self.Q[r]):
                moving[r], M[r] = True, compose(self.P[r], self.Q[r])
        return moving, M

    def accumulate(self, accum, frames, g, cam, naive=False):
        self._motion = self.motion()
        out = super().accumulate(accum, frames, g, cam, naive)
        self.P = list(self.Q)
        return out

    def _points(self, g, cam):
        """Steps 3 with the extension: x' per pixel (H, W, 3), whatever the pixel's guide says."""
        moving, M = self._motion
        idp = guide_id(g)
        with np.errstate(all="ignore"):
            x = (np.asarray(g["t"], F)[..., None] * pixel_dirs(cam, self.W, self.H) + cam[0]).astype(F)
            if len(moving):
                posed = (idp != MISS) & (idp < len(moving))
                r = np.where(posed, idp, 0).astype(np.int64)
                m = M[r]  # (H, W, 3, 4)
                xm = np.stack([((m[..., i, 0] * x[..., 0] + m[..., i, 1] * x[..., 1]) + m[..., i, 2] * x[..., 2]) + m[..., i, 3]
                               for i in range(3)], -1).astype(F)
                x = np.where((posed & moving[r])[..., None], xm, x)
        return x

    def _vector(self, C, g, cam):
        W, H, P = self.W, self.H, self.prev
        out = np.empty((H, W, 4), F)
        out[..., :3], out[..., 3] = C, F1
        if P is None:
            return out
        idp = guide_id(g)
        n = np.asarray(g["normal"], F)
        po, pf, pr, pu = P["cam"]
        with np.errstate(all="ignore"):
            v = self._points(g, cam) - po
            a = dot3(v, pf) / dot3(pf, pf)
            b = dot3(v, pr) / dot3(pr, pr)
            c = dot3(v, pu) / dot3(pu, pu)
            uu = (b / a + FH) * F(W) - FH
            vv = (c / a + FH) * F(H) - FH
            assert a.dtype == F and uu.dtype == F
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

    def _naive(self, C, g, cam):
        W, H, P = self.W, self.H, self.prev
        out = np.empty((H, W, 4), F)
        out[..., :3], out[..., 3] = C, F1
        if P is None:
            return out
        moving, M = self._motion
        o, f, r, u = cam
        po, pf, pr, pu = P["cam"]
        du, dv = r / F(W), u / F(H)
        p00 = (((o + f) - r / F(2)) - u / F(2)) + FH * (du + dv)
        sdot = lambda a, b: (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]  # noqa: E731
        with np.errstate(all="ignore"):
            for j in range(H):
                for i in range(W):
                    if g["tri"][j, i] == MISS:  # before anything indexes the poses
                        continue
                    ident, n = int(g["bvh"][j, i]), g["normal"][j, i]
                    d = ((p00 + F(i) * du) + F(j) * dv) - o
                    x = F(g["t"][j, i]) * d + o
                    if ident < len(moving) and moving[ident]:
                        m = M[ident]
                        x = np.asarray([((m[k, 0] * x[0] + m[k, 1] * x[1]) + m[k, 2] * x[2]) + m[k, 3] for k in range(3)], F)
                    v = x - po
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


def posed_two_wall_guide(cam, W, H, frames=(IDENTITY, IDENTITY)):
    """temporal_ref.two_wall_guide with each record posed by its `frame` (world -> model): the ray goes through the
    frame as traversal.hpp's xform takes it and meets the wall in MODEL space, so `t` (the frame is affine: the
    ray's parameter is the same in both spaces) and the model-frame normal (0, 0, 1) come out as the query reports
    them.  Record 0: the back wall z = 0, |x| < 1.5, |y| < 1; record 1: the front square z = 1, |x - 0.3| < 0.4,
    |y| < 0.4.  The nearer hit wins.  Returns (tri, t, normal, bvh, model_xy); model_xy is the hit point's model x, y."""
    o = as_camera(cam)[0]
    d = pixel_dirs(cam, W, H)
    tri = np.full((H, W), MISS, np.uint32)
    t = np.full((H, W), 1e30, F)
    bvh = np.zeros((H, W), np.uint32)
    nrm = np.zeros((H, W, 3), F)
    mxy = np.zeros((H, W, 2), F)
    with np.errstate(all="ignore"):
        for z, rec, inside in ((F(0), 0, lambda x, y: (np.abs(x) < 1.5) & (np.abs(y) < 1.0)),
                               (F(1), 1, lambda x, y: (np.abs(x - F(0.3)) < 0.4) & (np.abs(y) < 0.4))):
            to, td = xform(frames[rec], o, 1.0), xform(frames[rec], d, 0.0)
            s = ((z - to[2]) / td[..., 2]).astype(F)
            x, y = to[0] + s * td[..., 0], to[1] + s * td[..., 1]
            hit = (s > 0) & inside(x, y) & (s < t)
            tri[hit], bvh[hit], t[hit] = 7 + rec, rec, s[hit]
            nrm[hit] = (0, 0, 1)
            mxy[hit] = np.stack([x, y], -1)[hit]
    return tri, t, nrm, bvh, mxy


def interior(mask):
    """Pixels whose 3 x 3 neighbourhood lies in `mask` (outside the image counts as outside the mask)."""
    H, W = mask.shape
    padded = np.zeros((H + 2, W + 2), bool)
    padded[1:-1, 1:-1] = mask
    m = np.ones((H, W), bool)
    for oy in (0, 1, 2):
        for ox in (0, 1, 2):
            m &= padded[oy:oy + H, ox:ox + W]
    return m


# position, yaw, pitch: temporal_ref's two-wall cameras (the first two equal, then three small moves)
CAMERAS = [((0, 0, 4), -90, 0), ((0, 0, 4), -90, 0), ((.15, .05, 3.9), -92, 1), ((.3, .1, 3.8), -94, 2),
           ((-.4, 0, 3.8), -84, -1)]


def square_poses():
    """Per frame of CAMERAS the poses (wall, square): the wall stands still; the square stands still for a frame,
    translates twice, then turns 10 degrees about z under a non-uniform scale."""
    still = pose_from_model(IDENTITY)
    moves = [column_major(), column_major(), column_major(translation=(.1, .05, 0)), column_major(translation=(.2, .05, .1)),
             column_major(rotation("z", 10.0) @ np.diag([1.1, 0.9, 1.0]), (.2, .05, .1))]
    return [(still, pose_from_model(m)) for m in moves]


def moving_two_wall_frames(w, h, seed=11):
    """Per frame: (camera vectors, accumulation as a sum over 3 frames, guide fields (tri, t, normal, bvh), poses)."""
    rng = np.random.default_rng(seed + 1000 * w + h)
    frames = []
    for (pos, yaw, pitch), poses in zip(CAMERAS, square_poses()):
        cam = T.camera_vectors(pos, yaw, pitch)
        accum = np.ones((h, w, 4), F)
        accum[..., :3] = rng.uniform(0, 6, (h, w, 3)).astype(F)
        fields = posed_two_wall_guide(cam, w, h, [p[0] for p in poses])[:4]
        frames.append((cam, accum, fields, poses))
    return frames
