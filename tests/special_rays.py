"""Deterministic ray sets at the special values of the slab and triangle tests, for tests/test_special_rays_cpu.py
(the oracle alone: the conditions that make the sets meaningful) and tests/test_gpu_special_rays.py (the kernels).

Every generator takes a Scene whose first BVH record has the identity frame (rays are in that model's space) and
returns (rays, labels): a RAY_DTYPE array and an equally long array of strings "family/kind", so a failing ray names
its family.  float32 throughout; a seeded default_rng; a few thousand rays per family at most.

Also here: the numpy restatement of IntersectsBox (oracle/srt_oracle.c intersects_box, with fmin / fmax for the
oracle's fmn / fmx) over every node of a scene, and of xform.
"""
import numpy as np

import srt_amd as S
from oracle import pyoracle as O

MISS = 0xFFFFFFFF
INF_T = np.float32(1e30)
F = np.float32
T_MIN = F(0.00001)  # IntersectsTriangle: t > 0.00001f
A_MIN = F(0.0001)   # IntersectsTriangle: a > -0.0001f && a < 0.0001f is parallel
DENORM_MIN = np.nextafter(F(0), F(1))
# one direction component is replaced by each of these (special_values); 2^-127 is a denormal with a finite reciprocal
D_SPECIALS = [F(0.0), F(-0.0), F(np.inf), F(-np.inf), F(np.nan), DENORM_MIN, -DENORM_MIN, F(1e-39), F(2.0 ** -126),
              F(2.0 ** -127), F(2.0 ** 126), F(-2.0 ** 126), F(3e38)]
O_SPECIALS = [F(np.inf), F(-np.inf), F(np.nan), F(3e38)]
T_SPECIALS = [F(np.inf), F(np.nan), F(0.0), F(-1.0), F(-np.inf), DENORM_MIN]


def family_of(labels):
    return np.array([s.split("/")[0] for s in labels])


def _labels(n, text):
    return np.full(n, text, dtype="U40")


def _rays(o, d, t=INF_T):
    rays = np.zeros(len(o), S.RAY_DTYPE)
    rays["o"], rays["d"], rays["t"] = np.asarray(o, F), np.asarray(d, F), t
    return rays


def root_box(scene):
    r = scene.nodes[int(scene.bvhs[0]["first_index"])]
    return r["min"].astype(np.float64), r["max"].astype(np.float64)


def box_planes(scene):
    """Per axis, the distinct min / max coordinates of the scene's nodes (float32)."""
    return [np.unique(np.concatenate([scene.nodes["min"][:, a], scene.nodes["max"][:, a]])) for a in range(3)]


def features(scene):
    """Triangle corners, then edge midpoints (float32 arithmetic), [n, 3] each."""
    c = scene.verts["pos"][scene.tris["v"]].astype(F)  # [n_tris, 3, 3]
    mid = np.concatenate([(c[:, i] + c[:, (i + 1) % 3]) * F(0.5) for i in range(3)])
    return c.reshape(-1, 3), mid.astype(F)


def sphere_rays(lo, hi, n, seed, spread=1.7):
    """Generic rays (tests/test_gpu_queries.py has the same): origins on a sphere around the box, aimed at points
    jittered inside the box scaled by `spread`."""
    rng = np.random.default_rng(seed)
    c, half = (lo + hi) / 2, (hi - lo) / 2
    v = rng.normal(size=(n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    o = (c + 2.0 * np.linalg.norm(hi - lo) * v).astype(F)
    tgt = c + rng.uniform(-1, 1, size=(n, 3)) * half * spread
    return _rays(o, (tgt - o.astype(np.float64)).astype(F))


def triangle_rays(scene, n, seed):
    """Rays aimed at random points inside random triangles from a few triangle sizes away: they find a scene that
    fills little of its bounding box (a chain of triangles over many orders of magnitude)."""
    rng = np.random.default_rng(seed)
    c = scene.verts["pos"][scene.tris["v"][rng.integers(0, len(scene.tris), n)]].astype(np.float64)
    p = (c * rng.dirichlet((1, 1, 1), n)[:, :, None]).sum(1)
    v = rng.normal(size=(n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    size = np.linalg.norm(c[:, 1] - c[:, 0], axis=1) + np.linalg.norm(c[:, 2] - c[:, 0], axis=1)
    o = (p + v * (size * rng.uniform(2.0, 6.0, n))[:, None]).astype(F)
    return _rays(o, (p - o.astype(np.float64)).astype(F))


def hitting_rays(scene, n, seed):
    """The first n rays the oracle hits of sphere_rays followed by triangle_rays, with each one's triangle and
    distance (on a compact model the sphere_rays alone suffice)."""
    lo, hi = root_box(scene)
    cand = np.concatenate([sphere_rays(lo, hi, 4 * n + 64, seed, spread=0.9), triangle_rays(scene, 8 * n, seed)])
    tri, t, _, _ = O.Oracle(scene).trace_closest(1, cand)
    k = np.flatnonzero(tri != MISS)[:n]
    assert len(k) == n, "too few generic rays hit the scene"
    return cand[k], tri[k], t[k]


def _outside(rng, lo, hi, axis, sign, n):
    """Coordinates on `axis` outside [lo, hi], on the side a ray travelling with `sign` comes from."""
    ext = hi[axis] - lo[axis]
    m = rng.uniform(1.0, 4.0, n) * (1.0 + 0.05 * ext)
    return np.where(sign > 0, lo[axis] - m, hi[axis] + m)


def on_plane_axis(scene, n=2400, seed=101):
    """Axis-parallel rays: +-1 on one axis, a zero of either sign on the other two, whose origin coordinates lie on
    box planes of those axes; the origin is outside the root box along the travelling axis."""
    rng = np.random.default_rng(seed)
    lo, hi = root_box(scene)
    planes = box_planes(scene)
    i = np.arange(n)
    axis, sign = i % 3, np.where((i // 3) % 2 == 0, 1.0, -1.0)
    zs = [np.where((i // 6) % 2 == 0, F(0.0), F(-0.0)), np.where((i // 12) % 2 == 0, F(0.0), F(-0.0))]
    o, d = np.zeros((n, 3), F), np.zeros((n, 3), F)
    for a in range(3):
        m = axis == a
        o[m, a] = _outside(rng, lo, hi, a, sign[m], m.sum()).astype(F)
        d[m, a] = sign[m]
        for j, b in enumerate(((a + 1) % 3, (a + 2) % 3)):
            o[m, b] = rng.choice(planes[b], m.sum())
            d[m, b] = zs[j][m]
    return _rays(o, d), _labels(n, "on_plane_axis/axis")


def on_plane_one_zero(scene, n=2400, seed=102):
    """One direction component is a zero of either sign and the origin's coordinate on that axis lies on a box
    plane; the other two components are generic and point into the model."""
    rng = np.random.default_rng(seed)
    lo, hi = root_box(scene)
    planes = box_planes(scene)
    rays = sphere_rays(lo, hi, n, seed, spread=0.8)
    i = np.arange(n)
    for a in range(3):
        m = i % 3 == a
        rays["o"][m, a] = rng.choice(planes[a], m.sum())
        rays["d"][m, a] = np.where((i[m] // 3) % 2 == 0, F(0.0), F(-0.0))
    return rays, _labels(n, "on_plane_one_zero/one_zero")


def axis_onto_features(scene, n=3000, seed=103):
    """Axis-parallel rays from p + 32 e along -e, p a triangle corner or an edge midpoint: shared edges and corners,
    u == 0, v == 0, u + v == 1, and distance ties across leaves."""
    rng = np.random.default_rng(seed)
    corners, mids = features(scene)
    p = np.concatenate([corners[rng.integers(0, len(corners), n // 2)], mids[rng.integers(0, len(mids), n - n // 2)]])
    i = np.arange(n)
    e = np.zeros((n, 3), F)
    e[i, i % 3] = np.where((i // 3) % 2 == 0, F(1.0), F(-1.0))
    o = (p + F(32.0) * e).astype(F)
    lab = np.where(i < n // 2, "axis_onto_features/corner", "axis_onto_features/midpoint").astype("U40")
    return _rays(o, -e), lab


def feature_targets(scene, n=2000, seed=104):
    """Generic origins aimed exactly at triangle corners and edge midpoints."""
    rng = np.random.default_rng(seed)
    lo, hi = root_box(scene)
    corners, mids = features(scene)
    p = np.concatenate([corners[rng.integers(0, len(corners), n // 2)], mids[rng.integers(0, len(mids), n - n // 2)]])
    o = sphere_rays(lo, hi, n, seed)["o"]
    lab = np.where(np.arange(n) < n // 2, "feature_targets/corner", "feature_targets/midpoint").astype("U40")
    return _rays(o, (p - o).astype(F)), lab


def _ulps(x, k):
    """x moved by k units in the last place (x > 0, finite)."""
    return (np.asarray(x, F).view(np.int32) + np.int32(k)).view(F)


ULP_STEPS = (0, 1, -1, 16, -16)


def epsilon_t(scene, n_base=400, seed=105, with_near=False):
    """Hitting rays whose origin is moved along the ray until the hit distance is 0.00001f or one of its neighbours
    (+-1, +-16 ulp): the strict `t > 0.00001f`.  And the rays as they are, their intersection_distance 16 ulp under
    and over the hit distance, and at 0.00001f's neighbours (the window (0.00001, t) closes).
    with_near: also return the triangle each ray's unmoved original hits (the near triangle)."""
    base, tri, t = hitting_rays(scene, n_base, seed)
    o64, d64 = base["o"].astype(np.float64), base["d"].astype(np.float64)
    out, lab, near = [], [], []
    for k in ULP_STEPS:
        target = float(_ulps(T_MIN, k))
        r = base.copy()
        r["o"] = (o64 + (t.astype(np.float64) - target)[:, None] * d64).astype(F)
        out.append(r)
        near.append(tri)
        lab.append(_labels(n_base, f"epsilon_t/t_min{k:+d}ulp"))
    q = n_base // 4
    for k in (16, -16):
        r = base[:q].copy()
        r["t"] = _ulps(t[:q], k)
        out.append(r)
        near.append(tri[:q])
        lab.append(_labels(q, f"epsilon_t/tmax{k:+d}ulp"))
    for k in (0, 1, 16):
        r = out[0][:q].copy()  # the near triangle is at about 0.00001f
        r["t"] = _ulps(T_MIN, k)
        out.append(r)
        near.append(tri[:q])
        lab.append(_labels(q, f"epsilon_t/tmax_at_t_min{k:+d}ulp"))
    if with_near:
        return np.concatenate(out), np.concatenate(lab), np.concatenate(near)
    return np.concatenate(out), np.concatenate(lab)


def mt_a(scene, tri, d):
    """Moller-Trumbore's a = dot(e1, cross(d, e2)) of triangle tri[i] for direction d[i], in float64."""
    c = scene.verts["pos"][scene.tris["v"][tri]].astype(np.float64)
    e1, e2 = c[:, 1] - c[:, 0], c[:, 2] - c[:, 0]
    with np.errstate(all="ignore"):
        return np.einsum("ij,ij->i", e1, np.cross(np.asarray(d, np.float64), e2))


HUGE_A = 2.0 ** 126  # from here on the reciprocal of `a` is a division (traversal.hpp tri_prep)


def parallel_threshold(scene, n_base=250, seed=106, with_near=False):
    """Hitting rays whose direction is scaled (the query API takes unnormalised ones) until a of the hit triangle
    lands on +-0.0001f, the scale searched a few ulp either way so both sides of the threshold occur; the same rays
    with very short and very long directions; and axis-parallel rays from far away with directions so long that
    1.0 / a is a denormal while the hit distance stays above 0.00001.
    with_near: also return the triangle each ray was made for."""
    base, tri, _ = hitting_rays(scene, n_base, seed)
    a = mt_a(scene, tri, base["d"])
    out, lab, near = [], [], []
    s0 = (float(A_MIN) / np.abs(a)).astype(F)
    for k in (0, 1, -1, 2, -2, 4, -4):
        r = base.copy()
        r["d"] = (base["d"] * _ulps(s0, k)[:, None]).astype(F)
        out.append(r)
        near.append(tri)
        lab.append(_labels(n_base, f"parallel_threshold/scale{k:+d}ulp"))
    for e in (-60, -20, 20, 60, 100, 120):
        r = base[: n_base // 2].copy()
        with np.errstate(over="ignore"):
            r["d"] = (r["d"] * F(2.0 ** e)).astype(F)
        out.append(r)
        near.append(tri[: n_base // 2])
        lab.append(_labels(len(r), f"parallel_threshold/length2^{e}"))
    # far axis-parallel rays onto points inside triangles: d = -D e with |a| = D |n_e| in [2^126, 2^128), o = p + S e
    # with t = S / D = 2^-13 (p's own coordinate on the axis is far below S's ulp)
    rng = np.random.default_rng(seed)
    c = scene.verts["pos"][scene.tris["v"]].astype(np.float64)
    nrm = np.cross(c[:, 1] - c[:, 0], c[:, 2] - c[:, 0])
    m = 4 * n_base
    ti = rng.integers(0, len(c), m)
    ax = np.argmax(np.abs(nrm[ti]), axis=1)
    w = rng.dirichlet((1, 1, 1), m)
    p = (c[ti] * w[:, :, None]).sum(1)
    big = 2.0 ** rng.uniform(126.05, 127.9, m) / np.abs(nrm[ti, ax])
    ok = big < 3e38
    sign = np.where(rng.integers(0, 2, m) == 0, 1.0, -1.0)
    e = np.zeros((m, 3))
    e[np.arange(m), ax] = sign
    o = p.copy()
    o[np.arange(m), ax] = sign * big * 2.0 ** -13
    far = _rays(o[ok].astype(F), (-e[ok] * big[ok, None]).astype(F))
    out.append(far)
    near.append(ti[ok].astype(np.uint32))
    lab.append(_labels(len(far), "parallel_threshold/huge_a"))
    if with_near:
        return np.concatenate(out), np.concatenate(lab), np.concatenate(near)
    return np.concatenate(out), np.concatenate(lab)


def _robust_hitting_rays(scene, n, seed):
    """Rays from near the model that the oracle hits, preferring those that still hit with any one direction
    component zeroed (so the zero-like specials of special_values leave rays that hit)."""
    rng = np.random.default_rng(seed)
    lo, hi = root_box(scene)
    ext = np.maximum(hi - lo, 0.1 * (hi - lo).max())
    m = 64 * n
    o = rng.uniform(lo - 0.3 * ext, hi + 0.3 * ext, size=(m, 3)).astype(F)
    tgt = (lo + hi) / 2 + rng.uniform(-0.3, 0.3, size=(m, 3)) * (hi - lo)
    cand = np.concatenate([_rays(o, (tgt - o.astype(np.float64)).astype(F)), triangle_rays(scene, m, seed)])
    orc = O.Oracle(scene)
    hit = orc.trace_closest(1, cand)[0] != MISS
    kept = np.zeros(len(cand), int)
    for a in range(3):
        z = cand.copy()
        z["d"][:, a] = 0.0
        kept += orc.trace_closest(1, z)[0] != MISS
    k = np.flatnonzero(hit)
    k = k[np.argsort(-kept[k], kind="stable")][:n]
    assert len(k) == n, "too few rays hit the scene"
    return cand[k]


def special_values(scene, n_base=32, seed=107):
    """Rays the oracle hits with one field replaced at a time: a component of d by each of D_SPECIALS, a component
    of o by each of O_SPECIALS, t by each of T_SPECIALS; the all-zero direction; and pairs of specials."""
    base = _robust_hitting_rays(scene, n_base, seed)
    out, lab = [], []

    def put(r, text):
        out.append(r)
        lab.append(_labels(len(r), "special_values/" + text))

    for field, specials in (("d", D_SPECIALS), ("o", O_SPECIALS)):
        for j, v in enumerate(specials):
            for a in range(3):
                r = base.copy()
                r[field][:, a] = v
                put(r, f"{field}{a}#{j}")
    for j, v in enumerate(T_SPECIALS):
        r = base.copy()
        r["t"] = v
        put(r, f"t#{j}")
    r = base.copy()
    r["d"] = F(0.0)
    put(r, "d_all_zero")
    # pairs: two components of d, d with o, d with t
    pairs = [(F(0.0), F(-0.0)), (F(0.0), F(np.inf)), (F(np.inf), F(-np.inf)), (F(np.nan), F(0.0)),
             (DENORM_MIN, F(2.0 ** 126)), (F(-0.0), F(3e38)), (F(2.0 ** -126), F(-2.0 ** 126))]
    for j, (u, v) in enumerate(pairs):
        for a in range(3):
            r = base.copy()
            r["d"][:, a], r["d"][:, (a + 1) % 3] = u, v
            put(r, f"pair_dd{a}#{j}")
            r = base.copy()
            r["d"][:, a], r["o"][:, a] = u, v  # e.g. a zero direction with an infinite origin on the same axis
            put(r, f"pair_do{a}#{j}")
    for j, (u, v) in enumerate([(F(0.0), F(np.inf)), (F(-0.0), F(np.nan)), (F(np.inf), F(0.0)), (F(np.nan), F(np.inf))]):
        r = base.copy()
        r["d"][:, j % 3], r["t"] = u, v
        put(r, f"pair_dt#{j}")
    return np.concatenate(out), np.concatenate(lab)


FAMILIES = (on_plane_axis, on_plane_one_zero, axis_onto_features, feature_targets, epsilon_t, parallel_threshold,
            special_values)


def mixed_wave(scene, per_family=290, seed=108, sets=None):
    """The families interleaved ray by ray with generic rays: special, generic, special, ... with the specials taken
    round-robin from the families, so one 64-lane wave holds lanes on the division fallbacks beside lanes that are
    not, and lanes that finish at once beside lanes that walk the tree."""
    sets = sets if sets is not None else [f(scene) for f in FAMILIES]
    rng = np.random.default_rng(seed)
    picks = [rng.choice(len(r), min(per_family, len(r)), replace=False) for r, _ in sets]
    k = min(len(p) for p in picks)
    special = np.stack([r[p[:k]] for (r, _), p in zip(sets, picks)], axis=1).reshape(-1)
    slab = np.stack([l[p[:k]] for (_, l), p in zip(sets, picks)], axis=1).reshape(-1)
    lo, hi = root_box(scene)
    generic = sphere_rays(lo, hi, len(special), seed)
    rays = np.stack([special, generic], axis=1).reshape(-1)
    lab = np.stack([np.char.add("mixed_wave/", family_of(slab)).astype("U40"), _labels(len(special), "mixed_wave/generic")],
                   axis=1).reshape(-1)
    return rays, lab


def all_families(scene):
    """{family name: (rays, labels)} of every family and mixed_wave."""
    sets = [f(scene) for f in FAMILIES]
    out = {f.__name__: s for f, s in zip(FAMILIES, sets)}
    out["mixed_wave"] = mixed_wave(scene, sets=sets)
    return out


def concat(sets):
    return np.concatenate([r for r, _ in sets]), np.concatenate([l for _, l in sets])


# ---------------------------------------------------------------------------
# numpy restatements
# ---------------------------------------------------------------------------
def xform(frame, v, w):
    """oracle xform: ((m0 x + m4 y) + m8 z) + m12 w per row, float32, in that order."""
    m = np.asarray(frame, F).reshape(16)
    v = np.asarray(v, F)
    with np.errstate(all="ignore"):
        return np.stack([((m[r] * v[:, 0] + m[4 + r] * v[:, 1]) + m[8 + r] * v[:, 2]) + m[12 + r] * F(w)
                         for r in range(3)], axis=1).astype(F)


def slab_terms(scene, o, d):
    """(min - o) * (1 / d) and (max - o) * (1 / d) for every ray and every node: two float32 [rays, nodes, 3]."""
    mn, mx = scene.nodes["min"].astype(F), scene.nodes["max"].astype(F)
    o, d = np.asarray(o, F), np.asarray(d, F)
    with np.errstate(all="ignore"):
        inv = (F(1.0) / d).astype(F)
        t0 = (mn[None] - o[:, None]) * inv[:, None]
        t1 = (mx[None] - o[:, None]) * inv[:, None]
    return t0, t1


def nan_slab(scene, o, d, chunk=512):
    """Per ray: does a NaN occur in a slab term of some node?"""
    out = np.zeros(len(o), bool)
    for s in range(0, len(o), chunk):
        t0, t1 = slab_terms(scene, o[s:s + chunk], d[s:s + chunk])
        out[s:s + chunk] = (np.isnan(t0) | np.isnan(t1)).any(axis=(1, 2))
    return out


def intersects_box(t0, t1, lo=np.fmin, hi=np.fmax):
    """intersects_box from the slab terms on: (tn, tf, the returned distance).  `lo` / `hi`: the min / max used
    (np.fmin / np.fmax return the other operand for a NaN, as the oracle's fmn / fmx do)."""
    with np.errstate(all="ignore"):
        tmin, tmax = lo(t0, t1), hi(t0, t1)
        tn = hi(hi(tmin[..., 0], tmin[..., 1]), tmin[..., 2])
        tf = lo(lo(tmax[..., 0], tmax[..., 1]), tmax[..., 2])
        ret = np.where(tn <= tf, np.where(tn >= 0, tn, tf), F(np.inf))
    return tn, tf, ret


def accept_oracle(ret, dist):
    """Intersects: b < dist && !isinf(b)."""
    with np.errstate(all="ignore"):
        return (ret < dist) & ~np.isinf(ret)


def accept_three_term(tn, tf, dist):
    """traversal.hpp box_test: b = tn >= 0 ? tn : tf; (tn <= tf) & (b < dist) & (b != -inf)."""
    with np.errstate(all="ignore"):
        b = np.where(tn >= 0, tn, tf)
        return (tn <= tf) & (b < dist) & (b != -np.inf)


# ---------------------------------------------------------------------------
# two records of one model: a translated frame and a permuted one
# ---------------------------------------------------------------------------
# World -> model translation of record 0.  On Rubik o - T and (o - T) + T are exact in float32 for every box-plane
# coordinate o (T is a multiple of each one's ulp and o - T stays in o's binade or a finer one), so an origin on a
# box plane in model space is on it again after xform (tests/test_special_rays_cpu.py checks it).
TRANSLATION = (F(0.5), F(0.5), F(0.25))


def frame_translate():
    m = np.eye(4, dtype=F)
    m[3, :3] = TRANSLATION  # glm column 3
    return m.reshape(16)


def frame_permute():
    """model = (world.z, world.x, -world.y): every row of xform has two products with a zero entry, so a zero
    direction component arrives as a sum of signed zeros and an infinite one turns the other rows into NaN."""
    m = np.zeros(16, F)
    m[8 + 0], m[0 + 1], m[4 + 2], m[15] = 1.0, 1.0, -1.0, 1.0
    return m


def world_for_translate(rays):
    w = rays.copy()
    with np.errstate(all="ignore"):
        w["o"] = rays["o"] - np.asarray(TRANSLATION, F)
    return w


def world_for_permute(rays):
    w = rays.copy()
    for f in ("o", "d"):
        w[f] = np.stack([rays[f][:, 1], -rays[f][:, 2], rays[f][:, 0]], axis=1)
    return w
