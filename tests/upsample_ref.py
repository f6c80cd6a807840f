"""An independent numpy float32 restatement of the guided upsampling of include/srt_upsample.h (DESIGN.md section 5,
"Guided upsampling"), for the tests and for tools/upsample_grid.py.  It never calls into the library.

The operation only uses + - * /, max, abs, comparisons and integer arithmetic in fp32, in source order, so numpy
float32 arithmetic reproduces the kernel bit for bit.  `upsample` is the gathered-array form; `upsample_naive` is a
per-pixel scalar loop of the same definition, used to cross-check the first on small images.  Both also return, per
full pixel, which path produced it: BILINEAR, RING or NEAREST.  Guides are denoise_ref.make_guide dictionaries.
"""
from __future__ import annotations

import numpy as np

import denoise_ref as D

MISS = D.MISS
F0, F1 = np.float32(0.0), np.float32(1.0)
BILINEAR, RING, NEAREST = 0, 1, 2


def ids(g):
    """id(g): the BVH record's bits on a hit, all ones on a miss."""
    return np.where(g["tri"] == MISS, np.uint32(MISS), g["bvh"]).astype(np.uint32)


def axis_terms(n_full, f):
    """(i0, a0, a1) of the full coordinates 0 .. n_full - 1: n = 2X + 1 - f, i0 = floor(n / 2f), r = n - 2f * i0,
    a1 = float(r) / float(2f), a0 = 1 - a1."""
    X = np.arange(n_full, dtype=np.int64)
    n = 2 * X + 1 - f
    i0 = np.floor_divide(n, 2 * f)
    r = n - 2 * f * i0
    a1 = r.astype(np.float32) / np.float32(2 * f)
    a0 = F1 - a1
    assert a1.dtype == np.float32 and a0.dtype == np.float32
    return i0, a0, a1


def _stage(C, fin, idl, gl, idP, gP, I0, J0, taps, sd, nsq):
    """One stage over `taps` = [(dx, dy, k or None)]: (sw, sum, number of accepted taps, smallest accepted weight).
    k None: the ring's weights."""
    h, w = idl.shape
    hitP = idP != MISS
    nP, tP = gP["normal"], gP["t"]
    sw = np.zeros(idP.shape, np.float32)
    sm = np.zeros(idP.shape + (3,), np.float32)
    cnt = np.zeros(idP.shape, np.int32)
    wmin = np.full(idP.shape, np.inf, np.float32)
    for dx, dy, k in taps:
        qi, qj = np.broadcast_arrays(I0 + dx, J0 + dy)
        inside = (qi >= 0) & (qi < w) & (qj >= 0) & (qj < h)
        ci, cj = np.clip(qi, 0, w - 1), np.clip(qj, 0, h - 1)
        Cq, nq, tq = C[cj, ci], gl["normal"][cj, ci], gl["t"][cj, ci]
        valid = inside & (idl[cj, ci] == idP) & fin[cj, ci]
        wn = np.maximum((nP[..., 0] * nq[..., 0] + nP[..., 1] * nq[..., 1]) + nP[..., 2] * nq[..., 2], F0)
        for _ in range(nsq):
            wn = wn * wn
        xz = np.abs(tP - tq) / (sd * (tP + tq))
        wz = F1 / ((F1 + xz) * (F1 + xz))
        if k is None:
            wgt = np.where(hitP, wn * wz, F1).astype(np.float32)
        else:
            wgt = np.where(hitP, (k * wn) * wz, k).astype(np.float32)
        take = valid & (wgt > 0)
        sm = np.where(take[..., None], sm + wgt[..., None] * Cq, sm)
        sw = np.where(take, sw + wgt, sw)
        cnt = cnt + take
        wmin = np.where(take, np.minimum(wmin, wgt), wmin)
    assert sw.dtype == np.float32 and sm.dtype == np.float32
    return sw, sm, cnt, wmin


def upsample(accum, frames, low_guide, full_guide, f, normal_squarings=5, sigma_depth=0.2, detail=False):
    """(out (H, W, 3) float32, path (H, W) uint8) from the low accumulation image (h, w, 4), a SUM over `frames`.  With
    `detail` a third value: {"taps": accepted taps of the stage that decided the pixel (0: nearest), "min_weight": the
    smallest of their weights (inf: nearest)}."""
    C = D.mean_colour(accum, frames)
    h, w = C.shape[:2]
    H, W = f * h, f * w
    assert full_guide["tri"].shape == (H, W) and low_guide["tri"].shape == (h, w)
    sd = np.float32(sigma_depth)
    fin = np.isfinite(C).all(-1)
    idl, idP = ids(low_guide), ids(full_guide)
    i0, a0, a1 = axis_terms(W, f)
    j0, b0, b1 = axis_terms(H, f)
    I0, J0 = i0[None, :], j0[:, None]
    a, b = (a0[None, :], a1[None, :]), (b0[:, None], b1[:, None])
    with np.errstate(all="ignore"):
        bil = [(dx, dy, (a[dx] * b[dy]).astype(np.float32)) for dy in (0, 1) for dx in (0, 1)]
        sw, sm, bn, bw = _stage(C, fin, idl, low_guide, idP, full_guide, I0, J0, bil, sd, normal_squarings)
        ring = [(dx, dy, None) for dy in (-1, 0, 1, 2) for dx in (-1, 0, 1, 2)]
        rw, rm, rn, rmin = _stage(C, fin, idl, low_guide, idP, full_guide, I0, J0, ring, sd, normal_squarings)
        Y, X = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        near = C[Y // f, X // f]
        out = np.where((sw > 0)[..., None], sm / sw[..., None], np.where((rw > 0)[..., None], rm / rw[..., None], near))
    path = np.where(sw > 0, BILINEAR, np.where(rw > 0, RING, NEAREST)).astype(np.uint8)
    assert out.dtype == np.float32
    if detail:
        return out, path, {"taps": np.where(sw > 0, bn, np.where(rw > 0, rn, 0)),
                           "min_weight": np.where(sw > 0, bw, np.where(rw > 0, rmin, np.float32(np.inf)))}
    return out, path


def upsample_naive(accum, frames, low_guide, full_guide, f, normal_squarings=5, sigma_depth=0.2):
    """The same definition, one pixel and one tap at a time in scalar np.float32 (slow: small images only)."""
    C = D.mean_colour(accum, frames)
    h, w = C.shape[:2]
    H, W = f * h, f * w
    sd = np.float32(sigma_depth)
    idl, idP = ids(low_guide), ids(full_guide)
    out = np.zeros((H, W, 3), np.float32)
    path = np.zeros((H, W), np.uint8)

    def terms(X):
        n = 2 * X + 1 - f
        i0 = n // (2 * f)
        a1 = np.float32(n - 2 * f * i0) / np.float32(2 * f)
        return i0, (F1 - a1, a1)

    with np.errstate(all="ignore"):
        for Y in range(H):
            for X in range(W):
                i0, a = terms(X)
                j0, b = terms(Y)
                pid, nP, tP = idP[Y, X], full_guide["normal"][Y, X], full_guide["t"][Y, X]

                def stage(taps):
                    sw, sm = F0, [F0] * 3
                    for dx, dy, k in taps:
                        qi, qj = i0 + dx, j0 + dy
                        if not (0 <= qi < w and 0 <= qj < h) or idl[qj, qi] != pid or not np.isfinite(C[qj, qi]).all():
                            continue
                        if pid != MISS:
                            nq, tq = low_guide["normal"][qj, qi], low_guide["t"][qj, qi]
                            dot = (nP[0] * nq[0] + nP[1] * nq[1]) + nP[2] * nq[2]
                            wn = dot if dot > 0 else F0
                            for _ in range(normal_squarings):
                                wn = wn * wn
                            xz = np.abs(tP - tq) / (sd * (tP + tq))
                            wz = F1 / ((F1 + xz) * (F1 + xz))
                            wgt = wn * wz if k is None else (k * wn) * wz
                        else:
                            wgt = F1 if k is None else k
                        if not wgt > 0:
                            continue
                        sm = [sm[c] + wgt * C[qj, qi, c] for c in range(3)]
                        sw = sw + wgt
                    return sw, sm

                sw, sm = stage([(dx, dy, a[dx] * b[dy]) for dy in (0, 1) for dx in (0, 1)])
                if not sw > 0:
                    path[Y, X] = RING
                    sw, sm = stage([(dx, dy, None) for dy in (-1, 0, 1, 2) for dx in (-1, 0, 1, 2)])
                if sw > 0:
                    out[Y, X] = [sm[c] / sw for c in range(3)]
                else:
                    path[Y, X] = NEAREST
                    out[Y, X] = C[Y // f, X // f]
    return out, path


def replicate(img, f):
    """Each low pixel as an f x f block: nearest-neighbour upsampling."""
    return np.repeat(np.repeat(img, f, axis=0), f, axis=1)
