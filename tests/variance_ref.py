"""An independent numpy float32 restatement of include/srt_variance.h ("Variance-guided
filter"): the temporal luminance moments and the variance-guided a-trous filter, for the tests and for
tools/variance_sigma_grid.py.  It never calls into the library.

Only + - * /, min, abs, floor, comparisons and the float32 square root are used, in fp32 and in source order, so
numpy float32 arithmetic reproduces the kernels bit for bit.  `VarianceTemporalRef.accumulate_moments`, `resolve`
and `one_pass` are the shifted-array forms; `resolve_naive` and `one_pass_naive` are per-pixel scalar loops of the
same definition, used to cross-check the first on small images.
"""
from __future__ import annotations

import numpy as np

import denoise_ref as D
import temporal_motion_ref as M
from temporal_ref import F, F0, F1, FH, MISS, as_camera, dot3, guide_id

LR, LG, LB = F(0.2126), F(0.7152), F(0.0722)
EPS_L = F(1e-4)
KG = (F(0.5), F(0.25))  # per axis: the 3 x 3 blur's 1/4, 1/8, 1/16 are products of these


def lum(c):
    return (LR * c[..., 0] + LG * c[..., 1]) + LB * c[..., 2]


def pos_or_zero(d):
    """d > 0 ? d : 0 -- a NaN gives 0."""
    return np.where(d > 0, d, F0).astype(F)


# ---------------------------------------------------------------------------------------------------------------
# 1. temporal moments
# ---------------------------------------------------------------------------------------------------------------
class VarianceTemporalRef(M.TemporalMotionRef):
    """temporal_motion_ref's object (without poses it is temporal_ref's) with the moment history next to it."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.mom = None          # (H, W, 2): m1 | m2 of the previous frame
        self.mom_valid = False

    def reset(self):
        super().reset()
        self.mom_valid = False

    def accumulate(self, accum, frames, g, cam, naive=False):
        out = super().accumulate(accum, frames, g, cam, naive)
        self.mom_valid = False   # a plain call leaves no moments of this frame
        return out

    def _taps(self, g, cam, P):
        """Steps 3-6 of srt_temporal.h: per tap (take, wb, qy, qx), dy outer, dx inner."""
        W, H = self.W, self.H
        idp = guide_id(g)
        n = np.asarray(g["normal"], F)
        po, pf, pr, pu = P["cam"]
        v = self._points(g, cam) - po
        a = dot3(v, pf) / dot3(pf, pf)
        b = dot3(v, pr) / dot3(pr, pr)
        c = dot3(v, pu) / dot3(pu, pu)
        uu = (b / a + FH) * F(W) - FH
        vv = (c / a + FH) * F(H) - FH
        ok = (idp != MISS) & (a > 0) & (uu >= -1) & (uu < F(W)) & (vv >= -1) & (vv < F(H))
        fu, fv = np.floor(uu), np.floor(vv)
        i0 = np.where(ok, fu, F0).astype(np.int64)
        j0 = np.where(ok, fv, F0).astype(np.int64)
        fx, fy = uu - fu, vv - fv
        taps = []
        for dy in (0, 1):
            for dx in (0, 1):
                qx, qy = i0 + dx, j0 + dy
                inside = (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
                qx, qy = np.clip(qx, 0, W - 1), np.clip(qy, 0, H - 1)
                wb = ((fx if dx else F1 - fx) * (fy if dy else F1 - fy)).astype(F)
                take = ok & inside & (P["id"][qy, qx] == idp)
                take &= dot3(n, P["normal"][qy, qx]) >= self.normal_min
                take &= np.abs(a - P["t"][qy, qx]) <= self.depth_tol * (a + P["t"][qy, qx])
                take &= np.isfinite(P["col"][qy, qx]).all(-1) & (wb > 0)
                taps.append((take, wb, qy, qx))
        return taps

    def accumulate_moments(self, accum, frames, g, cam, naive=False):
        """(out, moments): out as `accumulate` gives it, moments (H, W, 4) = (m1, m2, v, N)."""
        P, had_moments = self.prev, self.mom_valid
        camv = as_camera(cam)
        self._motion = self.motion()
        C = (np.asarray(accum, F)[..., :3] / F(frames)).astype(F)
        with np.errstate(all="ignore"):
            L = lum(C)
            m1, m2, N = L.copy(), (L * L).astype(F), np.ones(L.shape, F)
            if P is not None and had_moments:
                sw, s1, s2 = np.zeros(L.shape, F), np.zeros(L.shape, F), np.zeros(L.shape, F)
                Nh = np.full(L.shape, np.inf, F)
                for take, wb, qy, qx in self._taps(g, camv, P):
                    sw = np.where(take, sw + wb, sw)
                    s1 = np.where(take, s1 + wb * self.mom[qy, qx, 0], s1)
                    s2 = np.where(take, s2 + wb * self.mom[qy, qx, 1], s2)
                    Nh = np.where(take, np.minimum(Nh, P["N"][qy, qx]), Nh)
                has, cfin = sw > 0, np.isfinite(C).all(-1)
                h1, h2 = s1 / sw, s2 / sw
                Np = np.minimum(Nh + F1, self.max_history)
                k = F1 / Np
                m1 = np.where(has & cfin, h1 + k * (L - h1), np.where(has, h1, m1)).astype(F)
                m2 = np.where(has & cfin, h2 + k * (L * L - h2), np.where(has, h2, m2)).astype(F)
                N = np.where(has & cfin, Np, np.where(has, Nh, F1)).astype(F)
            v = pos_or_zero(m2 - m1 * m1)
        out = M.TemporalMotionRef.accumulate(self, accum, frames, g, camv, naive)
        self.mom, self.mom_valid = np.stack([m1, m2], -1), True
        mom = np.stack([m1, m2, v, N], -1)
        assert mom.dtype == F
        return out, mom


# ---------------------------------------------------------------------------------------------------------------
# 2. the variance-guided filter
# ---------------------------------------------------------------------------------------------------------------
def _neighbour(g, ox, oy, nsq, sd):
    """For the tap at offset (ox, oy): (same, wn, wz) -- inside the image with p's id (both hits), and the normal
    and depth weights of srt_denoise.h's filter."""
    hit = g["tri"] != MISS
    n, t = g["normal"], g["t"]
    inside = D._shift(np.ones(hit.shape, bool), ox, oy, False)
    same = hit & inside & D._shift(hit, ox, oy, False) & (D._shift(g["bvh"], ox, oy, 0) == g["bvh"])
    nq, tq = D._shift(n, ox, oy, 0), D._shift(t, ox, oy, 0)
    wn = np.maximum((n[..., 0] * nq[..., 0] + n[..., 1] * nq[..., 1]) + n[..., 2] * nq[..., 2], F0)
    for _ in range(nsq):
        wn = wn * wn
    xz = np.abs(t - tq) / (sd * (t + tq))
    wz = F1 / ((F1 + xz) * (F1 + xz))
    return same, wn.astype(F), wz.astype(F)


def resolve(colour, frames, g, moments, min_history=4, normal_squarings=5, sigma_depth=0.2):
    """(C_0, var_0) from the colour sum, the guide and the moments (H, W, 4)."""
    C0 = D.mean_colour(colour, frames)
    mom = np.asarray(moments, F)
    hit = g["tri"] != MISS
    mh, sd = F(min_history), F(sigma_depth)
    s1, s2, sw = (np.zeros(hit.shape, F) for _ in range(3))
    with np.errstate(all="ignore"):
        for dy in range(-3, 4):
            for dx in range(-3, 4):
                same, wn, wz = _neighbour(g, dx, dy, normal_squarings, sd)
                mq = D._shift(mom, dx, dy, 0)
                take = same & np.isfinite(mq[..., 0]) & np.isfinite(mq[..., 1])
                w = wn * wz
                s1 = np.where(take, s1 + w * mq[..., 0], s1)
                s2 = np.where(take, s2 + w * mq[..., 1], s2)
                sw = np.where(take, sw + w, sw)
        a, b = s1 / sw, s2 / sw
        spatial = np.where(sw > 0, pos_or_zero(b - a * a) * (mh / mom[..., 3]), F0)
        var0 = np.where(hit, np.where(mom[..., 3] >= mh, mom[..., 2], spatial), F0).astype(F)
    assert C0.dtype == F and var0.dtype == F
    return C0, var0


def one_pass(C, var, g, step, sigma_lum=1.0, sigma_depth=0.2, normal_squarings=5):
    """(C_{i+1}, var_{i+1}) from (C_i, var_i) at step 2^i."""
    sl_, sd = F(sigma_lum), F(sigma_depth)
    hit = g["tri"] != MISS
    with np.errstate(all="ignore"):
        sg, sk = np.zeros(hit.shape, F), np.zeros(hit.shape, F)
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                same = _neighbour(g, dx, dy, 0, sd)[0]
                vq = D._shift(var, dx, dy, 0)
                take = same & np.isfinite(vq)
                kg = KG[abs(dx)] * KG[abs(dy)]
                sg = np.where(take, sg + kg * vq, sg)
                sk = np.where(take, sk + kg, sk)
        gb = np.where(sk > 0, sg / sk, F0).astype(F)
        sl = sl_ * np.sqrt(gb) + EPS_L
        Lp = lum(C)
        lfin = np.isfinite(Lp)
        sw, sv = np.zeros(hit.shape, F), np.zeros(hit.shape, F)
        sm = np.zeros(C.shape, F)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                ox, oy = dx * step, dy * step
                same, wn, wz = _neighbour(g, ox, oy, normal_squarings, sd)
                Cq, vq = D._shift(C, ox, oy, 0), D._shift(var, ox, oy, 0)
                xl = np.abs(Lp - lum(Cq)) / sl
                wl = np.where(lfin, F1 / ((F1 + xl) * (F1 + xl)), F1).astype(F)
                k = D.H_TAPS[abs(dx)] * D.H_TAPS[abs(dy)]
                w = ((k * wn) * wz) * wl
                take = same & np.isfinite(Cq).all(-1) & (w > 0)
                sw = np.where(take, sw + w, sw)
                sm = np.where(take[..., None], sm + w[..., None] * Cq, sm)
                sv = np.where(take & np.isfinite(vq), sv + (w * w) * vq, sv)
        got = hit & (sw > 0)
        out = np.where(got[..., None], sm / sw[..., None], C)
        vout = np.where(got, sv / (sw * sw), np.where(hit, var, F0))
    assert out.dtype == F and vout.dtype == F and sl.dtype == F
    return out, vout


def run_variance(colour, frames, g, moments, passes=5, normal_squarings=5, sigma_depth=0.2, sigma_lum=1.0,
                 min_history=4, naive=False):
    """(C_passes (H, W, 3), var_passes (H, W)): what srt_denoise_run_variance writes."""
    assert passes >= 1
    res, step = (resolve_naive, one_pass_naive) if naive else (resolve, one_pass)
    C, var = res(colour, frames, g, moments, min_history, normal_squarings, sigma_depth)
    for i in range(passes):
        C, var = step(C, var, g, 1 << i, sigma_lum, sigma_depth, normal_squarings)
    return C, var


# -- one pixel and one tap at a time ------------------------------------------------------------------------------
def _wn_wz(g, y, x, qy, qx, nsq, sd):
    a, b = g["normal"][y, x], g["normal"][qy, qx]
    dot = (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]
    wn = dot if dot > 0 else F0
    for _ in range(nsq):
        wn = wn * wn
    tp, tq = g["t"][y, x], g["t"][qy, qx]
    xz = np.abs(tp - tq) / (sd * (tp + tq))
    return wn, F1 / ((F1 + xz) * (F1 + xz))


def _same(g, y, x, qy, qx):
    h, w = g["tri"].shape
    return 0 <= qx < w and 0 <= qy < h and g["tri"][qy, qx] != MISS and g["bvh"][qy, qx] == g["bvh"][y, x]


def resolve_naive(colour, frames, g, moments, min_history=4, normal_squarings=5, sigma_depth=0.2):
    C0 = D.mean_colour(colour, frames)
    mom = np.asarray(moments, F)
    h, w = g["tri"].shape
    mh, sd = F(min_history), F(sigma_depth)
    var0 = np.zeros((h, w), F)
    with np.errstate(all="ignore"):
        for y in range(h):
            for x in range(w):
                if g["tri"][y, x] == MISS:
                    continue
                if mom[y, x, 3] >= mh:
                    var0[y, x] = mom[y, x, 2]
                    continue
                s1, s2, sw = F0, F0, F0
                for dy in range(-3, 4):
                    for dx in range(-3, 4):
                        qx, qy = x + dx, y + dy
                        if not _same(g, y, x, qy, qx) or not np.isfinite(mom[qy, qx, :2]).all():
                            continue
                        wn, wz = _wn_wz(g, y, x, qy, qx, normal_squarings, sd)
                        wgt = wn * wz
                        s1, s2, sw = s1 + wgt * mom[qy, qx, 0], s2 + wgt * mom[qy, qx, 1], sw + wgt
                if sw > 0:
                    a, b = s1 / sw, s2 / sw
                    d = b - a * a
                    var0[y, x] = (d if d > 0 else F0) * (mh / mom[y, x, 3])
    return C0, var0


def one_pass_naive(C, var, g, step, sigma_lum=1.0, sigma_depth=0.2, normal_squarings=5):
    h, w = g["tri"].shape
    sl_, sd = F(sigma_lum), F(sigma_depth)
    out, vout = C.copy(), np.zeros((h, w), F)
    with np.errstate(all="ignore"):
        for y in range(h):
            for x in range(w):
                if g["tri"][y, x] == MISS:
                    continue
                sg, sk = F0, F0
                for dy in (-1, 0, 1):
                    for dx in (-1, 0, 1):
                        qx, qy = x + dx, y + dy
                        if not _same(g, y, x, qy, qx) or not np.isfinite(var[qy, qx]):
                            continue
                        kg = KG[abs(dx)] * KG[abs(dy)]
                        sg, sk = sg + kg * var[qy, qx], sk + kg
                gb = sg / sk if sk > 0 else F0
                sl = sl_ * np.sqrt(gb) + EPS_L
                cp = C[y, x]
                Lp = (LR * cp[0] + LG * cp[1]) + LB * cp[2]
                lfin = bool(np.isfinite(Lp))
                sw, sv, sm = F0, F0, [F0] * 3
                for dy in range(-2, 3):
                    for dx in range(-2, 3):
                        qx, qy = x + dx * step, y + dy * step
                        if not _same(g, y, x, qy, qx):
                            continue
                        cq = C[qy, qx]
                        if not np.isfinite(cq).all():
                            continue
                        wl = F1
                        if lfin:
                            xl = np.abs(Lp - ((LR * cq[0] + LG * cq[1]) + LB * cq[2])) / sl
                            wl = F1 / ((F1 + xl) * (F1 + xl))
                        wn, wz = _wn_wz(g, y, x, qy, qx, normal_squarings, sd)
                        wgt = (((D.H_TAPS[abs(dx)] * D.H_TAPS[abs(dy)]) * wn) * wz) * wl
                        if not wgt > 0:
                            continue
                        sw = sw + wgt
                        sm = [sm[c] + wgt * cq[c] for c in range(3)]
                        if np.isfinite(var[qy, qx]):
                            sv = sv + (wgt * wgt) * var[qy, qx]
                if sw > 0:
                    out[y, x] = [sm[c] / sw for c in range(3)]
                    vout[y, x] = sv / (sw * sw)
                else:
                    vout[y, x] = var[y, x]
    return out, vout


# -- metrics of the quality comparison ------------------------------------------------------------------------------
def mse(img, truth, mask):
    return float(np.mean((np.asarray(img, np.float64)[mask] - np.asarray(truth, np.float64)[mask]) ** 2))


def tonemap(x):
    """x / (1 + x) per channel, in float64 (a metric, not part of the contract)."""
    x = np.asarray(x, np.float64)
    return x / (1.0 + x)


def mse_tm(img, truth, mask):
    return mse(tonemap(img), tonemap(truth), mask)
