"""Exact coordinates for the device texture samplers, CPU only (no library call that touches a device).

The surface stage takes the caller's ray and hit records.  A hit with t = 0 whose ray starts on its triangle's v0,
under an identity frame, has mp = (0 * td) + to = v0 exactly, so v0p = +0, d20 = d21 = +0 (the triangles here have
edges with no negative component), v = w = +0, u = 1 and s = (1 * uv0.x + 0 * uv1.x) + 0 * uv2.x: with the same uv on
all three vertices the sampler receives exactly that float (a NaN or an Inf arrives as NaN: 0 * inf).  `scene` builds
one such triangle per coordinate pair and `records` the rays and hits, so one launch delivers every chosen (s, t)
bit pattern to the kernel's sampler, and the attr record's uv field shows what arrived.

`sample64` is a float64 reference of the sampling contract written from the GL definition, not from
surface_ref.sample; its docstring derives the bound a float32 sampler must keep against it.
"""
from __future__ import annotations

import functools

import numpy as np

F = np.float32
E24 = 2.0 ** -24
# W x H x C of the texture set (array shapes are (H, W, C)); uploaded together, so every first-texel offset is in play
SHAPES = ((1, 1, 3), (1, 7, 3), (7, 1, 3), (2, 2, 4), (5, 3, 1), (3, 5, 2), (8, 8, 3), (64, 16, 4))
QNAN, QNAN_NEG = np.uint32(0x7FC00000), np.uint32(0xFFC00000)
EDGE = F(0.25)     # the lattice triangles: v0, v0 + (EDGE, 0, 0), v0 + (0, EDGE, 0)
COLUMNS = 64       # lattice columns; v0 = (1 + k % COLUMNS, 1 + k // COLUMNS, 0)


def _bits(u):
    return np.asarray([u], np.uint32).view(np.float32)[0]


def specials():
    """The float32 coordinates of no particular texture: zeros, ones, the wrap seam from both sides, whole numbers,
    coordinates whose fraction is 0 because they are huge, and the non-finite ones."""
    one = F(1)
    v = [F(0), F(-0.0), one, np.nextafter(one, F(0)), F(-1e-9), F(-2.0 ** -25), F(2.0 ** -149), F(-2.0 ** -149),
         F(-1), F(-1 + 2.0 ** -24), F(3), F(-3.25),
         F(2.0 ** 23 + 0.5), F(2.0 ** 24), F(-2.0 ** 24), F(1e20), F(-1e20), F(3.4e38), F(-3.4e38),
         _bits(QNAN), _bits(QNAN_NEG), F(np.inf), F(-np.inf)]
    return np.asarray(v, np.float32)


def _axis(n):
    """Per axis of n texels: the centres (i + 0.5) / n, and the seams i / n (i = 0 .. n) with the float32 neighbours
    one ulp either side of each."""
    i = np.arange(n, dtype=np.float32)
    centres = (i + F(0.5)) / F(n)
    seams = np.arange(n + 1, dtype=np.float32) / F(n)
    around = np.stack([np.nextafter(seams, F(-np.inf)), seams, np.nextafter(seams, F(np.inf))], 1).reshape(-1)
    assert centres.dtype == np.float32 and around.dtype == np.float32
    return centres, around


def coordinates(w, h):
    """The float32 (s, t) pairs for a w x h texture, an (n, 2) array: every texel centre; every seam and its two
    float32 neighbours, per i against ordinary t, per j against ordinary s, and seam against seam; the specials
    against each other, against ordinary values and against the first inner seam; 64 seeded uniform points in
    [-3, 3)^2."""
    cs, ss = _axis(w)
    ct, st = _axis(h)
    ordinary_s = np.asarray([cs[w // 2], F(0.3)], np.float32)   # a centre and a point that is neither centre nor seam
    ordinary_t = np.asarray([ct[h // 2], F(0.3)], np.float32)
    sp = specials()
    pairs = [np.stack(np.meshgrid(cs, ct, indexing="ij"), -1).reshape(-1, 2)]
    pairs.append(np.stack(np.meshgrid(ss, ordinary_t, indexing="ij"), -1).reshape(-1, 2))
    pairs.append(np.stack(np.meshgrid(ordinary_s, st, indexing="ij"), -1).reshape(-1, 2))
    m = max(len(ss), len(st))
    pairs.append(np.stack([np.resize(ss, m), np.resize(st, m)], -1))
    pairs.append(np.stack(np.meshgrid(sp, sp, indexing="ij"), -1).reshape(-1, 2))
    with_s = np.concatenate([ordinary_s, ss[3:6]])              # 1 / w and its neighbours
    with_t = np.concatenate([ordinary_t, st[3:6]])
    pairs.append(np.stack(np.meshgrid(sp, with_t, indexing="ij"), -1).reshape(-1, 2))
    pairs.append(np.stack(np.meshgrid(with_s, sp, indexing="ij"), -1).reshape(-1, 2))
    rng = np.random.default_rng(1000 * w + h)
    pairs.append(rng.uniform(-3, 3, (64, 2)).astype(np.float32))
    out = np.ascontiguousarray(np.concatenate(pairs).astype(np.float32))
    assert out.dtype == np.float32 and out.shape[1] == 2
    return out


@functools.lru_cache(maxsize=None)
def textures():
    """Seeded random bytes in SHAPES, no two equal in a row or a column of any channel: channel c of texel (i, j) is
    P_c[(i + k_c * j) mod 256] with P_c a random permutation of the bytes and k_c odd (i < 256 tells a row's texels
    apart, and an odd k_c is invertible mod 256, which tells a column's).  Left unchanged by every test."""
    rng = np.random.default_rng(20240521)
    out = []
    for w, h, c in SHAPES:
        t = np.zeros((h, w, c), np.uint8)
        jj, ii = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
        for ch in range(c):
            perm = rng.permutation(256).astype(np.uint8)
            k = 2 * int(rng.integers(8, 120)) + 1
            t[..., ch] = perm[(ii + k * jj) % 256]
        for ch in range(c):
            assert all(len(set(row)) == w for row in t[..., ch]) and all(len(set(col)) == h for col in t[..., ch].T)
        t.setflags(write=False)
        out.append(t)
    return tuple(out)


def _tree(lo_hi, max_leaf=4):
    """A NODE_DTYPE array over triangles 0 .. n-1 with the boxes `lo_hi` (n, 2, 3): a median split of the index
    range down to leaves of at most `max_leaf`, a node's children adjacent (first, first + 1), the root at 0."""
    import srt_amd as S

    n = len(lo_hi)
    nodes = [None]

    def fill(slot, a, b):
        lo, hi = lo_hi[a:b, 0].min(0), lo_hi[a:b, 1].max(0)
        if b - a <= max_leaf:
            nodes[slot] = (lo, a, hi, b - a)
            return
        first = len(nodes)
        nodes.extend([None, None])
        nodes[slot] = (lo, first, hi, 0)
        mid = (a + b) // 2
        fill(first, a, mid)
        fill(first + 1, mid, b)

    fill(0, 0, n)
    out = np.zeros(len(nodes), S.NODE_DTYPE)
    for k, (lo, first, hi, count) in enumerate(nodes):
        out[k] = (lo, first, hi, count)
    return out


def scene_from_triangles(texture_set, pos, uv, tex):
    """An srt_amd.Scene of len(pos) triangles built from arrays, as surface_scenes.textured_scene builds one:
    `pos` (n, 3, 3) and `uv` (n, 3, 2) per vertex, three vertices of its own per triangle; one sampled material per
    texture, material k pointing at handle k; triangle i uses material tex[i]; one BVH record with an identity
    frame over a tree of the triangles' boxes."""
    import srt_amd as S

    pos, uv = np.asarray(pos, np.float32), np.asarray(uv, np.float32)
    n = len(pos)
    verts = np.zeros(3 * n, S.VERT_DTYPE)
    verts["pos"], verts["uv"] = pos.reshape(-1, 3), uv.reshape(-1, 2)
    tris = np.zeros(n, S.TRI_DTYPE)
    tris["v"] = np.arange(3 * n, dtype=np.uint32).reshape(n, 3)
    tris["mat"] = np.broadcast_to(np.asarray(tex, np.uint32), (n,))
    mats = np.zeros(len(texture_set), S.MAT_DTYPE)
    mats["diffuse"], mats["Ks"], mats["Ns"], mats["use_texture"] = (1.0, 1.0, 1.0), (0.2, 0.2, 0.2), 10.0, 1
    mats["handle"][:, 0] = np.arange(len(texture_set))
    with np.errstate(all="ignore"):
        boxes = np.stack([np.fmin.reduce(pos, 1) - F(0.5), np.fmax.reduce(pos, 1) + F(0.5)], 1)
    nodes = _tree(boxes)
    bvhs = np.zeros(1, S.BVH_DTYPE)
    bvhs["count"] = len(nodes)
    bvhs["frame"][0] = np.eye(4, dtype=np.float32).reshape(16)
    return S.Scene(bvhs, nodes, mats, np.zeros((len(mats), 3), np.float32), tris, verts,
                   textures=[np.asarray(t) for t in texture_set], sample_textures=True,
                   tri_input=np.arange(n, dtype=np.uint32))


def scene(texture_set, coords, tex=0):
    """One small non-degenerate triangle per pair of `coords`, on a lattice (no two share a v0, no coordinate of a
    v0 is 0), all three vertices carrying that pair's uv; the triangles use the material of texture `tex` (an index,
    or one per pair)."""
    coords = np.asarray(coords, np.float32).reshape(-1, 2)
    k = np.arange(len(coords))
    v0 = np.stack([1 + k % COLUMNS, 1 + k // COLUMNS, np.zeros(len(k))], -1).astype(np.float32)
    pos = np.stack([v0, v0 + np.asarray([EDGE, 0, 0], np.float32), v0 + np.asarray([0, EDGE, 0], np.float32)], 1)
    uv = np.repeat(coords[:, None, :], 3, 1)
    return scene_from_triangles(texture_set, pos, uv, tex)


def records_at(scene, tri, origin, t):
    """RAY_DTYPE and HIT_DTYPE records of rays from `origin` down -z that hit triangle tri[i] at distance t[i]."""
    import srt_amd as S
    from srt_amd.query import HIT_DTYPE

    tri = np.asarray(tri, np.uint32)
    rays = np.zeros(len(tri), S.RAY_DTYPE)
    rays["o"], rays["d"], rays["t"] = origin, (0.0, 0.0, -1.0), F(1e30)
    hits = np.zeros(len(tri), HIT_DTYPE)
    hits["triangle"], hits["t"], hits["normal"] = tri, t, (0.0, 0.0, 1.0)
    hits["material"], hits["bvh"] = scene.tris["mat"][tri], 0
    return rays, hits


def records(scene):
    """The records that land ray k on v0 of triangle k at t = 0."""
    n = len(scene.tris)
    return records_at(scene, np.arange(n), scene.verts["pos"][scene.tris["v"][:, 0]], np.zeros(n, np.float32))


def sample64(texels, s, t):
    """texture(sampler2D, vec2(s, t)).xyz at level 0, GL_LINEAR, GL_REPEAT in float64, from the GL definition
    (OpenGL 4.6 section 8.14.2 wrap modes and 8.15.3 texture magnification): with the texture of w x h texels c / 255
    and u = frac(s) * w, i0 = floor(u - 0.5) mod w, i1 = (i0 + 1) mod w, alpha = frac(u - 0.5) (likewise j0, j1,
    beta from t and h), the result is (1 - alpha)(1 - beta) T[i0, j0] + alpha (1 - beta) T[i1, j0]
    + (1 - alpha) beta T[i0, j1] + alpha beta T[i1, j1].  T[i, j] is column i of row j: `texels` is (H, W, C), rows
    first.  Missing channels are 0; a 2-channel texture reads (r, g, 0).  The project's addition: a non-finite
    coordinate reads as 0.

    s and t are float32 and are taken exactly: a float32 is a float64, and frac is s - floor(s) there, off from
    the mathematical fraction by at most 2^-53 (a tiny negative s gives 1.0, which `mod` wraps as GL_REPEAT does).
    Returns (n, 3) float64.

    The bound a float32 sampler keeps against this, per channel.  e = 2^-24; a float32 result of size at most m
    rounds within m e (half an ulp of a value in [2^k, 2^(k+1)) is 2^k e), and one in [0, 1] within e / 2:
      * the input is exact;
      * frac = s - floor(s) lies in [0, 1]: one rounding, within e / 2;
      * u = frac * w: the error of frac grows to w e / 2, and the product, at most w, rounds within w e;
        x = u - 0.5, at most w in size, rounds within w e again.  So x is off by at most 2.5 w e, taken as 3 w e,
        and y by 3 h e;
      * the repeated bilinear surface is continuous in (x, y), across texel boundaries and across the wrap, and
        piecewise linear with slope at most max |T - T'| <= 1 per unit of x and of y: an error dx, dy in the
        coordinates moves the result by at most dx + dy, whichever texels floor() picks on either side;
      * alpha = x - floor(x) is exact for x >= 0 and one rounding (e / 2) for x in [-0.5, 0), which moves the result
        by at most e / 2, and likewise beta: e together;
      * 1 - alpha and 1 - beta round within e / 2 each; the weights are products of two factors in [0, 1]: w00 is
        off by at most e / 2 + e / 2 + e / 2, w10 and w01 by e, w11 by e / 2: 4 e together, against texels at most 1;
      * each texel c / 255 rounds within e / 2, under weights that sum to at most 1 + 4 e;
      * each product is at most its weight: the four roundings sum to at most e / 2 (1 + 4 e);
      * the three sums have partial results at most 1 + 4 e, which may lie in [1, 2): 3 e.
    The last five come to 9 e and a few e^2 (below 1e-6 e), which the charge of 3 w e for 2.5 w e covers:
    bound(w, h) = (3 w + 3 h + 9) * 2^-24.
    """
    tex = np.asarray(texels, np.uint8)
    if tex.ndim == 2:
        tex = tex[:, :, None]
    h, w, ch = tex.shape
    T = np.zeros((h, w, 3), np.float64)
    n = min(ch, 3)
    T[..., :n] = tex[..., :n].astype(np.float64) / 255.0
    s = np.asarray(s, np.float32).astype(np.float64)
    t = np.asarray(t, np.float32).astype(np.float64)
    s = np.where(np.isfinite(s), s, 0.0)
    t = np.where(np.isfinite(t), t, 0.0)
    x = (s - np.floor(s)) * w - 0.5
    y = (t - np.floor(t)) * h - 0.5
    i0 = np.floor(x).astype(np.int64) % w
    j0 = np.floor(y).astype(np.int64) % h
    i1, j1 = (i0 + 1) % w, (j0 + 1) % h
    alpha, beta = (x - np.floor(x))[..., None], (y - np.floor(y))[..., None]
    return (1 - alpha) * (1 - beta) * T[j0, i0] + alpha * (1 - beta) * T[j0, i1] \
        + (1 - alpha) * beta * T[j1, i0] + alpha * beta * T[j1, i1]


def bound(w, h):
    """The largest per-channel distance of a float32 sampler of the contract from sample64 (its docstring)."""
    return (3 * w + 3 * h + 9) * E24


# -- the second scene: triangles whose barycentric determinant is 0, underflows or overflows -------------------------

DEGENERATE = (
    # name, v0, v1, v2
    ("ordinary", (3.0, 2.0, 0.0), (4.0, 2.0, 0.0), (3.0, 3.5, 0.0)),
    ("collinear", (6.0, 2.0, 0.0), (7.0, 2.5, 0.0), (8.0, 3.0, 0.0)),
    ("two coincident", (10.0, 2.0, 0.0), (10.0, 2.0, 0.0), (11.0, 3.0, 0.0)),
    ("two coincident, v0 apart", (10.0, 5.0, 0.0), (11.0, 6.0, 0.0), (11.0, 6.0, 0.0)),
    ("a point", (13.0, 2.0, 0.0), (13.0, 2.0, 0.0), (13.0, 2.0, 0.0)),
    # d00, d01 and d11 are about 1e-24; their products, 1e-48, lie below half the smallest float32 and round to 0
    ("sliver, underflow", (0.0, 0.0, 0.0), (1e-12, 0.0, 0.0), (1e-12, 1e-14, 0.0)),
    # d11 = 1 + 1e-60 rounds to 1 = d00 = d01: the determinant cancels to 0
    ("sliver, cancellation", (16.0, 2.0, 0.0), (17.0, 2.0, 0.0), (17.0, 2.0 + 1e-30, 0.0)),
    # dots of 1e38 and 2e38 are finite, their products are not
    ("edges of 1e19", (2.0, 8.0, 0.0), (1e19, 8.0, 0.0), (1e19, 1e19, 0.0)),
    # dots of 4e38 are already infinite
    ("edges of 2e19", (2.0, 11.0, 0.0), (2e19, 11.0, 0.0), (0.0, 2e19, 0.0)),
)
DEGENERATE_UV = ((0.125, 0.25), (0.625, 0.375), (0.3125, 0.875))   # distinct per vertex


def degenerate_scene(texture_set, tex):
    """DEGENERATE's triangles with DEGENERATE_UV on their vertices, sampling texture `tex`; the records hit each on v0
    at t = 0 and, by a second ray from 2 above, at the mean of its vertices at t = 2.  Returns (scene, rays, hits)."""
    pos = np.asarray([[v0, v1, v2] for _, v0, v1, v2 in DEGENERATE], np.float32)
    n = len(pos)
    uv = np.broadcast_to(np.asarray(DEGENERATE_UV, np.float32), (n, 3, 2))
    sc = scene_from_triangles(texture_set, pos, uv, tex)
    with np.errstate(all="ignore"):
        mid = ((pos[:, 0] + pos[:, 1]) + pos[:, 2]) / F(3)
    tri = np.concatenate([np.arange(n), np.arange(n)])
    origin = np.concatenate([pos[:, 0], mid + np.asarray([0, 0, 2], np.float32)])
    t = np.concatenate([np.zeros(n, np.float32), np.full(n, 2, np.float32)])
    rays, hits = records_at(sc, tri, origin, t)
    return sc, rays, hits


# -- shared, computed once ------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def case(k):
    """Texture k of textures() over its coordinates(): {"tex", "coords", "scene", "rays", "hits", "want" (the
    restated attrs of the records), "terms" (surface_ref.shade's intermediate values)}.  Left unchanged."""
    import surface_ref as SR

    tex = textures()[k]
    coords = coordinates(tex.shape[1], tex.shape[0])
    sc = scene(textures(), coords, k)
    rays, hits = records(sc)
    terms = {}
    want = SR.shade(sc, rays, hits, textures=sc.textures, terms=terms)
    for a in (coords, rays, hits, want):
        a.setflags(write=False)
    return {"tex": tex, "coords": coords, "scene": sc, "rays": rays, "hits": hits, "want": want, "terms": terms}


SEAM_W, SEAM_H, SEAM_SPP, SEAM_DEPTH = 32, 24, 2, 2
_E = 2.0 ** -24
SEAM_UVS = (((0.0, 0.0), (1.0, 1.0)),                                      # seams on the quad's vertices
            ((-_E, -_E), (1.0 - _E, 1.0 - _E)),                            # the wrap seam from below
            ((2.0 ** 24, -2.0 ** 24), (2.0 ** 24 + 1, -2.0 ** 24 + 1)))    # no fraction left


@functools.lru_cache(maxsize=None)
def seam_setup(k):
    """surface_scenes.textured_setup at 32 x 24, depth 2, with the 8 x 8 random texture in place of the checker and
    the textured quad's uvs running from SEAM_UVS[k][0] to SEAM_UVS[k][1]."""
    import dataclasses

    import surface_scenes as SS

    setup = SS.textured_setup(SEAM_W, SEAM_H)
    sc = setup.scene
    (ls, lt), (hs, ht) = SEAM_UVS[k]
    verts = sc.verts.copy()
    verts["uv"][:4] = np.asarray([(ls, lt), (hs, lt), (hs, ht), (ls, ht)], np.float32)
    tex = list(sc.textures)
    tex[0] = np.asarray(textures()[SHAPES.index((8, 8, 3))])
    return dataclasses.replace(setup, scene=dataclasses.replace(sc, verts=verts, textures=tex), max_depth=SEAM_DEPTH)


@functools.lru_cache(maxsize=None)
def seam_oracle(k):
    """The oracle's (accumulation, output, stats) of seam_setup(k): reset + SEAM_SPP frames."""
    from conftest import oracle_render

    return oracle_render(seam_setup(k), SEAM_SPP)
