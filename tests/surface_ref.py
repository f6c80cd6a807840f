"""An independent numpy float32 restatement of the surface-attribute stage of include/srt_surface.h (DESIGN.md
section 5, "Surface attributes and demodulation"), for the tests and for tools/albedo_floor_grid.py.  It restates the
sampler itself and never calls into the library.

Everything is fp32 in source order: + - * / of numpy float32 are correctly rounded, and the one fused operation of
the contract, dot = fma(z, z', fma(y, y', x * x')), is `fma32`: the product is exact in float64, the sum is rounded to
odd there (Boldo & Melquiond: 53 >= 2 * 24 + 2 bits), and the final rounding to float32 is then the single rounding
of the exact a * b + c.
"""
from __future__ import annotations

import numpy as np

MISS = 0xFFFFFFFF
F = np.float32
ATTR_DTYPE = np.dtype([("albedo", "<f4", 3), ("bary_v", "<f4"), ("bary_w", "<f4"), ("uv", "<f4", 2), ("hit", "<u4")])
FLT_MAX = F(3.402823466e38)


def fma32(a, b, c):
    """fmaf(a, b, c) on float32 arrays (finite operands whose product neither overflows nor underflows float64)."""
    a, b, c = (np.asarray(v, np.float32).astype(np.float64) for v in (a, b, c))
    p = a * b                         # exact: 48 bits
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)     # TwoSum: s + e == p + c exactly
    odd = (s.view(np.int64) & 1) != 0
    toward = np.where(e > 0, np.inf, -np.inf)
    s = np.where((e != 0) & ~odd, np.nextafter(s, toward), s)  # round to odd
    return s.astype(np.float32)


def dot3(a, b):
    """pt_math.hpp's dot: fma(a.z, b.z, fma(a.y, b.y, a.x * b.x))."""
    return fma32(a[..., 2], b[..., 2], fma32(a[..., 1], b[..., 1], a[..., 0] * b[..., 0]))


def xform(m, v, w):
    """traversal.hpp's xform: ((m0 * x + m4 * y) + m8 * z) + m12 * w per row; m is (..., 16) column-major."""
    w = F(w)
    return np.stack([((m[..., r] * v[..., 0] + m[..., 4 + r] * v[..., 1]) + m[..., 8 + r] * v[..., 2]) + m[..., 12 + r] * w
                     for r in range(3)], axis=-1).astype(np.float32)


def as_rgb(texels):
    """(H, W, C) uint8 with C in 1..4 -> (H, W, 3): GL_RED reads (r, 0, 0), a 2-channel texture (r, g, 0)."""
    t = np.asarray(texels, np.uint8)
    if t.ndim == 2:
        t = t[:, :, None]
    out = np.zeros(t.shape[:2] + (3,), np.uint8)
    n = min(t.shape[2], 3)
    out[..., :n] = t[..., :n]
    return out


def sample_terms(texels, s, t):
    """`sample` with its intermediate values: {"nonfinite" (per axis), "frac", "x", "a", "i0", "i1" (each an (s, t)
    pair of arrays), "weights" (w00, w10, w01, w11), "out"}."""
    tex = as_rgb(texels)
    h, w = tex.shape[:2]
    s, t = np.asarray(s, np.float32).copy(), np.asarray(t, np.float32).copy()
    with np.errstate(all="ignore"):
        bad_s, bad_t = ~(np.abs(s) <= FLT_MAX), ~(np.abs(t) <= FLT_MAX)
        s[bad_s] = 0
        t[bad_t] = 0
        s = s - np.floor(s)
        t = t - np.floor(t)
        x, y = s * F(w) - F(0.5), t * F(h) - F(0.5)
        fx, fy = np.floor(x), np.floor(y)
        a, b = x - fx, y - fy
        i0, j0 = fx.astype(np.int64), fy.astype(np.int64)
        i1, j1 = i0 + 1, j0 + 1
        i0 = np.minimum(np.where(i0 < 0, w - 1, i0), w - 1)
        j0 = np.minimum(np.where(j0 < 0, h - 1, j0), h - 1)
        i1 = np.where(i1 >= w, 0, i1)
        j1 = np.where(j1 >= h, 0, j1)
        one = F(1)
        w00, w10, w01, w11 = (one - a) * (one - b), a * (one - b), (one - a) * b, a * b
        tx = tex.astype(np.float32) / F(255)
        out = ((w00[..., None] * tx[j0, i0] + w10[..., None] * tx[j0, i1]) + w01[..., None] * tx[j1, i0]) \
            + w11[..., None] * tx[j1, i1]
    assert out.dtype == np.float32
    return {"nonfinite": (bad_s, bad_t), "frac": (s, t), "x": (x, y), "a": (a, b), "i0": (i0, j0), "i1": (i1, j1),
            "weights": (w00, w10, w01, w11), "out": out}


def sample(texels, s, t):
    """texture(sampler2D, vec2(s, t)).xyz at level 0, GL_LINEAR, GL_REPEAT on arrays of coordinates: non-finite
    coordinates read as 0, texels are c / 255, the weighted texels are summed ((00 + 10) + 01) + 11."""
    return sample_terms(texels, s, t)["out"]


def shade(scene, rays, hits, *, textures=None, tex_albedo=None, bvh_count=None, frames=None, terms=None):
    """srt_surface_shade: ATTR_DTYPE records of RAY_DTYPE `rays` and HIT_DTYPE `hits` over `scene`'s arrays.
    `textures`: the uploaded set (list of (H, W, C) uint8); `tex_albedo`: (n_mats, 3) or None, srt_surface_create's
    argument; `frames`: (n_bvhs, 16) to override the scene's (update_model_matrix); `terms`: a dict that receives the
    intermediate values of the hit records ("idx", their positions, and "mp", "denom", "v", "w", "u")."""
    n = len(rays)
    out = np.zeros(n, ATTR_DTYPE)
    textures = textures or []
    n_bvhs = len(scene.bvhs)
    bvh_count = n_bvhs if bvh_count is None else bvh_count
    fr = np.zeros((n_bvhs + 1, 16), np.float32)
    fr[:n_bvhs] = scene.bvhs["frame"] if frames is None else frames
    tri = hits["triangle"].astype(np.int64)
    idx = np.nonzero(tri < len(scene.tris))[0]       # a miss is 0xFFFFFFFF
    if len(idx) == 0:
        return out
    tri = tri[idx]
    b = hits["bvh"][idx].astype(np.int64)
    m = fr[np.where((b < bvh_count) & (b < n_bvhs), b, n_bvhs)]
    with np.errstate(all="ignore"):
        to, td = xform(m, rays["o"][idx], 1), xform(m, rays["d"][idx], 0)
        mp = (hits["t"][idx][:, None] * td) + to
        tv = scene.tris["v"][tri]
        p0, p1, p2 = (scene.verts["pos"][tv[:, k]] for k in range(3))
        e1, e2 = p1 - p0, p2 - p0
        v0p = mp - p0
        d00, d01, d11 = dot3(e1, e1), dot3(e1, e2), dot3(e2, e2)
        d20, d21 = dot3(v0p, e1), dot3(v0p, e2)
        denom = F(1) / (d00 * d11 - d01 * d01)
        v = (d11 * d20 - d01 * d21) * denom
        w = (d00 * d21 - d01 * d20) * denom
        u = F(1) - v - w
        uv0, uv1, uv2 = (scene.verts["uv"][tv[:, k]] for k in range(3))
        uv = (u[:, None] * uv0 + v[:, None] * uv1) + w[:, None] * uv2
    if terms is not None:
        terms.update(idx=idx, mp=mp, denom=denom, v=v, w=w, u=u)
    mat = scene.mats[scene.tris["mat"][tri]]
    alb = mat["diffuse"].astype(np.float32).copy()
    sampled = mat["use_texture"] != 0
    if tex_albedo is not None:
        alb[sampled] = np.asarray(tex_albedo, np.float32)[scene.tris["mat"][tri]][sampled]
    else:
        handle = mat["handle"][:, 0].astype(np.uint64) | (mat["handle"][:, 1].astype(np.uint64) << np.uint64(32))
        alb[sampled] = 0
        for k, tex in enumerate(textures):
            sel = sampled & (handle == k)
            if sel.any():
                alb[sel] = sample(tex, uv[sel, 0], uv[sel, 1])
    assert uv.dtype == np.float32 and v.dtype == np.float32 and alb.dtype == np.float32
    out["albedo"][idx], out["bary_v"][idx], out["bary_w"][idx], out["uv"][idx], out["hit"][idx] = alb, v, w, uv, 1
    return out
