"""The exact-coordinate inputs of tests/test_gpu_surface_exact.py checked on the CPU (tests/surface_exact.py): the
injection through t = 0 hits on v0 is exact in the float32 restatement, the restated sampler equals
srt_texture_sample on every coordinate and stays within the derived bound of the float64 GL sampler, every class of
coordinate the device tests are about is populated, and the scenes' trees are trees the oracle traverses."""
import numpy as np
import pytest

import srt_amd as S
import surface_exact as X
import surface_ref as SR
from conftest import bits_equal

F = np.float32
TEXTURES = range(len(X.SHAPES))


def words(a):
    return np.ascontiguousarray(a).view(np.uint32)


def word(v):
    return int(np.asarray([v], np.float32).view(np.uint32)[0])


def test_the_texture_set():
    tex = X.textures()
    assert [(t.shape[1], t.shape[0], t.shape[2]) for t in tex] == list(X.SHAPES)
    for t in tex:                      # whole texels differ along every row and column (each channel does)
        for row in t:
            assert len({bytes(p) for p in row}) == t.shape[1]
        for col in t.transpose(1, 0, 2):
            assert len({bytes(p) for p in col}) == t.shape[0]


def test_coordinates_hold_what_the_device_tests_need():
    """The list itself, for the 5 x 3 texture: float32 pairs; centres, seams and their neighbours; the named specials
    on both axes, against each other and against ordinary values."""
    c = X.coordinates(5, 3)
    assert c.dtype == np.float32 and c.ndim == 2 and c.shape[1] == 2
    have = {(int(a), int(b)) for a, b in words(c)}
    key = lambda s, t: (word(s), word(t))  # noqa: E731
    for i in range(5):
        for j in range(3):
            assert key((F(i) + F(0.5)) / F(5), (F(j) + F(0.5)) / F(3)) in have
    s_all, t_all = set(words(c[:, 0]).tolist()), set(words(c[:, 1]).tolist())
    for n, axis in ((5, s_all), (3, t_all)):
        for i in range(n + 1):
            seam = F(i) / F(n)
            for v in (seam, np.nextafter(seam, F(-np.inf)), np.nextafter(seam, F(np.inf))):
                assert word(v) in axis
    named = [0.0, -0.0, 1.0, np.nextafter(F(1), F(0)), -1e-9, -2.0 ** -25, 2.0 ** -149, -1.0, -1 + 2.0 ** -24, 3.0,
             -3.25, 2.0 ** 23 + 0.5, 2.0 ** 24, -2.0 ** 24, 1e20, -1e20, 3.4e38]
    for v in named:
        assert word(v) in s_all and word(v) in t_all
        assert key(v, 0.3) in have and key(0.3, v) in have and key(v, -3.25) in have
    for nan in (X.QNAN, X.QNAN_NEG):
        assert int(nan) in s_all and int(nan) in t_all and (int(nan), word(0.3)) in have
        assert (word(0.3), int(nan)) in have
    inside = (np.abs(c) < 3).all(1)
    assert inside.sum() >= 64


@pytest.mark.parametrize("k", TEXTURES)
def test_injection_is_exact(k):
    """surface_ref.shade over records(scene): u = 1 and v = w = +0, so uv is the injected pair dword for dword where
    the component is finite (-0.0 and 2^-149 included) and NaN where it is not, and the albedo is the restated
    sample at exactly that pair."""
    c = X.case(k)
    coords, want, terms = c["coords"], c["want"], c["terms"]
    assert len(want) == len(coords) == len(terms["idx"]) and (want["hit"] == 1).all()
    assert (words(terms["v"]) == 0).all() and (words(terms["w"]) == 0).all() and (terms["u"] == 1).all()
    assert (terms["mp"] == c["rays"]["o"]).all()
    finite = np.isfinite(coords)
    assert (words(want["uv"])[finite] == words(coords)[finite]).all()
    assert np.isnan(want["uv"][~finite]).all() and (~finite).sum() > 40
    assert (words(want["bary_v"]) == 0).all() and (words(want["bary_w"]) == 0).all()
    direct = SR.sample(c["tex"], coords[:, 0], coords[:, 1])
    assert (words(want["albedo"]) == words(direct)).all() and np.isfinite(direct).all()


@pytest.mark.parametrize("k", TEXTURES)
def test_the_tree_is_one_the_oracle_traverses(k):
    """Rays dropped onto the inside of every lattice triangle find that triangle: the node array is a valid BVH."""
    from oracle import pyoracle as O

    sc = X.case(k)["scene"]
    n = len(sc.tris)
    rays = np.zeros(n, S.RAY_DTYPE)
    rays["o"] = sc.verts["pos"][sc.tris["v"][:, 0]] + np.asarray([0.0625, 0.0625, 1.0], np.float32)
    rays["d"], rays["t"] = (0.0, 0.0, -1.0), F(1e30)
    tri, t, _, _ = O.Oracle(sc).trace_closest(1, rays)
    assert (tri == np.arange(n)).all() and (t == 1).all()
    leaves = sc.nodes[sc.nodes["count"] > 0]
    assert leaves["count"].sum() == n and len(sc.nodes) > 1


@pytest.mark.parametrize("k", TEXTURES)
def test_restated_sampler_equals_srt_texture_sample(k):
    """tests/test_surface_api.py's comparison, on every coordinate of the new list: bit for bit."""
    c = X.case(k)
    got = SR.sample(c["tex"], c["coords"][:, 0], c["coords"][:, 1])
    want = np.stack([S.texture_sample(c["tex"], float(a), float(b)) for a, b in c["coords"]])
    bad = words(got) != words(want)
    print(f"{X.SHAPES[k]}: {int(bad.sum())} of {bad.size} components differ")
    assert not bad.any() and bits_equal(got, want).all()


@pytest.mark.parametrize("k", TEXTURES)
def test_restated_sampler_against_the_float64_sampler(k):
    c = X.case(k)
    w, h, _ = X.SHAPES[k]
    got = SR.sample(c["tex"], c["coords"][:, 0], c["coords"][:, 1]).astype(np.float64)
    err = np.abs(got - X.sample64(c["tex"], c["coords"][:, 0], c["coords"][:, 1])).max()
    print(f"{X.SHAPES[k]}: largest error {err / X.E24:.3f} * 2^-24, bound {X.bound(w, h) / X.E24:.0f} * 2^-24")
    assert err <= X.bound(w, h)


def test_sample64_reads_texel_centres_rows_and_wraps():
    """sample64 on its own: a centre is its texel (column i of row j), the seam between two texels their mean, and
    the wrap seam the mean of the last and the first; missing channels are 0."""
    tex = X.textures()[X.SHAPES.index((5, 3, 1))]
    t = tex[..., 0].astype(np.float64) / 255.0
    for i in range(5):
        for j in range(3):
            got = X.sample64(tex, F((i + 0.5) / 5), F((j + 0.5) / 3))
            assert abs(got[0] - t[j, i]) < 1e-7 and (got[1:] == 0).all()
    yc = F(1.5 / 3)
    assert abs(X.sample64(tex, F(2 / 5), yc)[0] - (t[1, 1] + t[1, 2]) / 2) < 1e-7
    for s in (0.0, 1.0, -1e-9, 3.0, 2.0 ** 24, np.nan, -np.inf):
        assert abs(X.sample64(tex, F(s), yc)[0] - (t[1, 4] + t[1, 0]) / 2) < 1e-7
    assert abs(X.sample64(tex, F(0.1), F(0))[0] - (t[2, 0] + t[0, 0]) / 2) < 1e-7


@pytest.mark.parametrize("k", TEXTURES)
def test_every_class_of_coordinate_is_populated(k):
    """From the restatement's intermediate values: texel centres (both fractions 0), seams (a fraction of exactly
    0.5), their neighbours on either side, s - floor(s) rounding to exactly 1.0f, a fraction of exactly 0 from a
    coordinate of 2^24 or more, and non-finite coordinates."""
    c = X.case(k)
    coords = c["coords"]
    w, h, _ = X.SHAPES[k]
    tm = SR.sample_terms(c["tex"], coords[:, 0], coords[:, 1])
    finite = np.isfinite(coords)
    assert (tm["nonfinite"][0] == ~finite[:, 0]).all() and (tm["nonfinite"][1] == ~finite[:, 1]).all()
    for axis, n in ((0, w), (1, h)):
        a, frac, ok = tm["a"][axis], tm["frac"][axis], finite[:, axis]
        huge = ok & (np.abs(coords[:, axis]) >= 2.0 ** 24)
        classes = {"centre": ok & ~huge & (a == 0) & (tm["a"][1 - axis] == 0),
                   "seam": ok & (a == F(0.5)),
                   "below a seam": ok & (a < F(0.5)) & (a > F(0.5) - n * 2.0 ** -22),
                   "above a seam": ok & (a > F(0.5)) & (a < F(0.5) + n * 2.0 ** -22),
                   "fraction 1.0f": ok & (frac == 1) & (coords[:, axis] < 0),
                   "fraction 0, huge": huge & (frac == 0),
                   "non-finite": tm["nonfinite"][axis]}
        for name, sel in classes.items():
            print(f"{X.SHAPES[k]} axis {axis}: {name}: {int(sel.sum())}")
            assert sel.any(), name
        # the wrap seam reads the last and the first texel, whichever side it is reached from
        wrap = classes["fraction 1.0f"] | classes["fraction 0, huge"]
        assert (tm["i0"][axis][wrap] == n - 1).all() and (tm["i1"][axis][wrap] == 0).all()
    assert ((tm["i0"][0] >= 0) & (tm["i0"][0] < w) & (tm["i1"][0] >= 0) & (tm["i1"][0] < w)).all()
    assert ((tm["i0"][1] >= 0) & (tm["i0"][1] < h) & (tm["i1"][1] >= 0) & (tm["i1"][1] < h)).all()


@pytest.mark.parametrize("k", TEXTURES)
def test_a_texel_centre_reads_its_texel(k):
    """Wherever the restatement's weights come out as (1, 0, 0, 0) at a centre, the result is that texel's c / 255
    exactly; on the power-of-two textures that is every centre (the issue asks for at least half)."""
    c = X.case(k)
    w, h, _ = X.SHAPES[k]
    n = w * h                                                    # coordinates() lists the centres first, s-major
    s, t = c["coords"][:n, 0], c["coords"][:n, 1]
    ii, jj = (g.reshape(-1) for g in np.meshgrid(np.arange(w), np.arange(h), indexing="ij"))
    assert (s == (ii.astype(np.float32) + F(0.5)) / F(w)).all() and (t == (jj.astype(np.float32) + F(0.5)) / F(h)).all()
    tm = SR.sample_terms(c["tex"], s, t)
    w00, w10, w01, w11 = tm["weights"]
    unit = (w00 == 1) & (w10 == 0) & (w01 == 0) & (w11 == 0)
    texel = SR.as_rgb(c["tex"])[jj, ii].astype(np.float32) / F(255)
    assert (tm["i0"][0][unit] == ii[unit]).all() and (tm["i0"][1][unit] == jj[unit]).all()
    assert (words(tm["out"][unit]) == words(texel[unit])).all()
    print(f"{X.SHAPES[k]}: {int(unit.sum())} of {n} centres have unit weights")
    if not (w & (w - 1)) and not (h & (h - 1)):
        assert 2 * unit.sum() >= n
        assert unit.all()                                        # (i + 0.5) / 2^k * 2^k - 0.5 is exact
    assert unit.any()


def test_degenerate_scene_reaches_the_divisions_by_zero():
    """The second scene, in the restatement: lanes with denom == inf, lanes with a NaN v, lanes with a finite
    result; the v0 hit of the ordinary triangle returns its uv0."""
    k = X.SHAPES.index((8, 8, 3))
    sc, rays, hits = X.degenerate_scene(X.textures(), k)
    terms = {}
    want = SR.shade(sc, rays, hits, textures=sc.textures, terms=terms)
    n = len(X.DEGENERATE)
    assert len(want) == 2 * n and (want["hit"] == 1).all()
    assert np.isposinf(terms["denom"]).sum() >= 8 and np.isnan(terms["v"]).sum() >= 8
    finite = np.isfinite(want["uv"]).all(1) & np.isfinite(want["bary_v"]) & np.isfinite(want["bary_w"])
    assert finite[0] and finite[n] and (want["uv"][0] == np.asarray(X.DEGENERATE_UV[0], np.float32)).all()
    assert 0 < want["bary_v"][n] < 1 and 0 < want["bary_w"][n] < 1
    assert np.isfinite(want["albedo"]).all()
    for name, lane in zip([d[0] for d in X.DEGENERATE], range(n)):
        print(f"{name}: denom {terms['denom'][lane]} / {terms['denom'][lane + n]}, v {terms['v'][lane]} / {terms['v'][lane + n]}")


def test_the_three_seam_frames_differ():
    """The path-tracer scenes of test_gpu_surface_exact.py, from the oracle alone: the three uv ranges give three
    different frames, and in each the textured quad is seen."""
    acc = [X.seam_oracle(k)[0] for k in range(len(X.SEAM_UVS))]
    for a in acc:
        assert a.shape == (X.SEAM_H, X.SEAM_W, 4) and np.isfinite(a[..., :3]).all()
    for i in range(3):
        for j in range(i + 1, 3):
            differ = ~bits_equal(acc[i], acc[j]).all(-1)
            print(f"frames {i} and {j}: {int(differ.sum())} of {differ.size} pixels differ")
            assert differ.sum() >= 20
    uv = X.seam_setup(2).scene.verts["uv"][:4]
    assert (uv[:, 0] == 2.0 ** 24).all() and set(uv[:, 1].tolist()) == {-2.0 ** 24, -2.0 ** 24 + 1}
