"""An independent numpy float32 restatement of the edge-avoiding filter of include/srt_denoise.h (DESIGN.md
section 5, "Denoiser"), for the tests and for tools/denoise_sigma_grid.py.  It never calls into the library.

The filter only uses + - * /, max, abs and comparisons in fp32, in source order, so numpy float32 arithmetic
reproduces the kernels bit for bit.  `atrous` is the shifted-array form; `atrous_naive` is a per-pixel scalar
loop of the same definition, used to cross-check the first on small images.
"""
from __future__ import annotations

import numpy as np

MISS = 0xFFFFFFFF
H_TAPS = (np.float32(0.375), np.float32(0.25), np.float32(0.0625))
F1 = np.float32(1.0)


def make_guide(tri, t, normal, bvh=None):
    """A guide as the filter reads it: (H, W) triangle ids, t, (H, W, 3) normals and BVH records."""
    tri = np.asarray(tri, np.uint32)
    return {"tri": tri, "t": np.asarray(t, np.float32), "normal": np.asarray(normal, np.float32),
            "bvh": np.zeros(tri.shape, np.uint32) if bvh is None else np.asarray(bvh, np.uint32)}


def guide_from_hits(hits, width, height):
    """HIT_DTYPE records (index j * W + i) as a guide."""
    sh = (height, width)
    return make_guide(hits["triangle"].reshape(sh), hits["t"].reshape(sh), hits["normal"].reshape(sh + (3,)),
                      hits["bvh"].reshape(sh))


def mean_colour(accum, frames):
    """C0 = accum.xyz / float(frames)."""
    return (np.asarray(accum, np.float32)[..., :3] / np.float32(frames)).astype(np.float32)


def _shift(a, ox, oy, fill):
    """b[y, x] = a[y + oy, x + ox] where that lies inside, else `fill`."""
    h, w = a.shape[:2]
    b = np.full_like(a, fill)
    x0, x1 = max(0, -ox), min(w, w - ox)
    y0, y1 = max(0, -oy), min(h, h - oy)
    if x0 < x1 and y0 < y1:
        b[y0:y1, x0:x1] = a[y0 + oy:y1 + oy, x0 + ox:x1 + ox]
    return b


def one_pass(C, g, step, sigma_c, sigma_depth, normal_squarings):
    sc, sd = np.float32(sigma_c), np.float32(sigma_depth)
    hit = g["tri"] != MISS
    fin = np.isfinite(C).all(-1)
    n, t = g["normal"], g["t"]
    sw = np.zeros(hit.shape, np.float32)
    sm = np.zeros(C.shape, np.float32)
    with np.errstate(all="ignore"):
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                ox, oy = dx * step, dy * step
                inside = _shift(np.ones(hit.shape, bool), ox, oy, False)
                hq = _shift(hit, ox, oy, False)
                bq = _shift(g["bvh"], ox, oy, 0)
                nq = _shift(n, ox, oy, 0)
                tq = _shift(t, ox, oy, 0)
                Cq = _shift(C, ox, oy, 0)
                valid = hit & inside & hq & (bq == g["bvh"]) & _shift(fin, ox, oy, False)
                k = H_TAPS[abs(dx)] * H_TAPS[abs(dy)]
                wn = np.maximum((n[..., 0] * nq[..., 0] + n[..., 1] * nq[..., 1]) + n[..., 2] * nq[..., 2],
                                np.float32(0))
                for _ in range(normal_squarings):
                    wn = wn * wn
                xz = np.abs(t - tq) / (sd * (t + tq))
                wz = F1 / ((F1 + xz) * (F1 + xz))
                d = C - Cq
                xc = ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]) / (sc * sc)
                wc = np.where(fin, F1 / ((F1 + xc) * (F1 + xc)), F1).astype(np.float32)
                w = ((k * wn) * wz) * wc
                take = valid & (w > 0)
                sw = np.where(take, sw + w, sw)
                sm = np.where(take[..., None], sm + w[..., None] * Cq, sm)
        out = np.where((hit & (sw > 0))[..., None], sm / sw[..., None], C)
    assert out.dtype == np.float32 and sw.dtype == np.float32
    return out


def atrous(C0, g, passes=5, normal_squarings=5, sigma_color=1.0, sigma_depth=0.05):
    """C_passes from C_0 (H, W, 3) float32 and a guide (make_guide)."""
    C = np.ascontiguousarray(C0, np.float32)
    for i in range(passes):
        C = one_pass(C, g, 1 << i, np.float32(sigma_color) * np.float32(2.0 ** -i), sigma_depth, normal_squarings)
    return C


def atrous_naive(C0, g, passes=5, normal_squarings=5, sigma_color=1.0, sigma_depth=0.05):
    """The same definition, one pixel and one tap at a time in scalar np.float32 (slow: small images only)."""
    C = np.ascontiguousarray(C0, np.float32)
    h, w = C.shape[:2]
    sd = np.float32(sigma_depth)
    with np.errstate(all="ignore"):
        for i in range(passes):
            s, sc = 1 << i, np.float32(sigma_color) * np.float32(2.0 ** -i)
            nxt = C.copy()
            for y in range(h):
                for x in range(w):
                    if g["tri"][y, x] == MISS:
                        continue
                    cp, np_, tp = C[y, x], g["normal"][y, x], g["t"][y, x]
                    pfin = bool(np.isfinite(cp).all())
                    sw, sm = np.float32(0), [np.float32(0)] * 3
                    for dy in range(-2, 3):
                        for dx in range(-2, 3):
                            qx, qy = x + dx * s, y + dy * s
                            if not (0 <= qx < w and 0 <= qy < h) or g["tri"][qy, qx] == MISS:
                                continue
                            cq = C[qy, qx]
                            if g["bvh"][qy, qx] != g["bvh"][y, x] or not np.isfinite(cq).all():
                                continue
                            nq, tq = g["normal"][qy, qx], g["t"][qy, qx]
                            k = H_TAPS[abs(dx)] * H_TAPS[abs(dy)]
                            dot = (np_[0] * nq[0] + np_[1] * nq[1]) + np_[2] * nq[2]
                            wn = dot if dot > 0 else np.float32(0)
                            for _ in range(normal_squarings):
                                wn = wn * wn
                            xz = np.abs(tp - tq) / (sd * (tp + tq))
                            wz = F1 / ((F1 + xz) * (F1 + xz))
                            wc = F1
                            if pfin:
                                d = cp - cq
                                xc = ((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]) / (sc * sc)
                                wc = F1 / ((F1 + xc) * (F1 + xc))
                            wgt = ((k * wn) * wz) * wc
                            if not wgt > 0:
                                continue
                            sw = sw + wgt
                            sm = [sm[c] + wgt * cq[c] for c in range(3)]
                    if sw > 0:
                        nxt[y, x] = [sm[c] / sw for c in range(3)]
            C = nxt
    return C


def camera_rays(origin, front, right, up, width, height):
    """tools/bench_queries.py::camera_rays on plain vectors: (o [3], d [H * W, 3]), index j * W + i, row 0 at
    the bottom."""
    o, front, right, up = (np.asarray(v, np.float32) for v in (origin, front, right, up))
    du, dv = right / np.float32(width), up / np.float32(height)
    p00 = (o + front - right / 2 - up / 2) + np.float32(0.5) * (du + dv)
    x, y = np.meshgrid(np.arange(width, dtype=np.float32), np.arange(height, dtype=np.float32))
    ps = p00 + x.reshape(-1, 1) * du + y.reshape(-1, 1) * dv
    return o, (ps - o).astype(np.float32)
