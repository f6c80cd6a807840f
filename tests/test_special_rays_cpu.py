"""CPU: the special-value ray sets of tests/special_rays.py, with the oracle alone.

What makes tests/test_gpu_special_rays.py meaningful is stated and checked here first: each family reaches the regime
it is named for (NaN slab terms, decisions that flip one ulp off the plane, both sides of each threshold, reciprocals
on the division fallback), on Rubik, within the oracle's own stack.  The bounds are floors with margin under what a
prototype of the generators measured with the oracle; if one fails, the generator is at fault, not the bound.

And the equivalence traversal.hpp's box_test claims -- its three-term accept against IntersectsBox followed by
`b < dist && !isinf(b)` -- is checked over every node for the on-plane rays, from a numpy restatement of
oracle/srt_oracle.c intersects_box with fmin / fmax (the oracle's fmn / fmx return the other operand for a NaN).
"""
import numpy as np
import pytest

import special_rays as SR
import srt_amd as S
from conftest import OBJECTS
from oracle import pyoracle as O

MISS = SR.MISS


@pytest.fixture(scope="module")
def rubik_scene():
    return S.Scene.from_models([S.load_obj(OBJECTS / "Rubik" / "Rubik.obj")])


@pytest.fixture(scope="module")
def families(rubik_scene):
    return SR.all_families(rubik_scene)


@pytest.fixture(scope="module")
def traced(rubik_scene, families):
    """{family: (triangle, t, stats)} of the oracle."""
    orc = O.Oracle(rubik_scene)
    out = {}
    for name, (rays, _) in families.items():
        tri, t, _, st = orc.trace_closest(1, rays)
        out[name] = (tri, t, st)
    return out


def nudged(rays):
    q = rays.copy()
    q["o"] = np.nextafter(rays["o"], np.float32(np.inf))
    return q


def test_sets_are_labelled_and_small(families):
    assert set(families) == {f.__name__ for f in SR.FAMILIES} | {"mixed_wave"}
    for name, (rays, labels) in families.items():
        assert rays.dtype == S.RAY_DTYPE and len(rays) == len(labels) and 0 < len(rays) <= 4500
        assert (SR.family_of(labels) == name).all()
    assert sum(len(r) for r, _ in families.values()) <= 24000


def test_generators_are_deterministic(rubik_scene, families):
    for f in SR.FAMILIES:
        rays, labels = f(rubik_scene)
        assert rays.tobytes() == families[f.__name__][0].tobytes() and (labels == families[f.__name__][1]).all()


def test_every_family_stays_inside_the_oracle_stack(traced):
    for name, (_, _, st) in traced.items():
        assert st["stack_overflow"] == 0, name


@pytest.mark.parametrize("name, nan_floor, change_floor", [("on_plane_axis", 1.0, 0.25), ("on_plane_one_zero", 1.0, 0.25),
                                                           ("axis_onto_features", 0.5, 0.25)])
def test_on_plane_rays_meet_nan_slab_terms_and_are_decision_dense(rubik_scene, families, traced, name, nan_floor,
                                                                    change_floor):
    rays, _ = families[name]
    tri = traced[name][0]
    has_nan = SR.nan_slab(rubik_scene, rays["o"], rays["d"])
    assert has_nan.mean() >= nan_floor  # 0 * inf at some node (1.0: every ray)
    tri_off = O.Oracle(rubik_scene).trace_closest(1, nudged(rays))[0]
    assert (tri_off != tri).mean() >= change_floor  # one ulp off the plane the oracle answers differently
    if name != "axis_onto_features":
        assert 0.20 <= (tri != MISS).mean() <= 0.85


def test_on_plane_axis_is_what_it_says(rubik_scene, families):
    rays, _ = families["on_plane_axis"]
    lo, hi = SR.root_box(rubik_scene)
    planes = SR.box_planes(rubik_scene)
    axis = np.argmax(np.abs(rays["d"]), axis=1)
    assert (np.abs(rays["d"]).sum(1) == 1.0).all()
    i = np.arange(len(rays))
    along, sign = rays["o"][i, axis], rays["d"][i, axis]
    assert (np.where(sign > 0, along < lo[axis], along > hi[axis])).all()  # outside the root box
    seen = set()
    for a in range(3):
        for b in ((a + 1) % 3, (a + 2) % 3):
            m = axis == a
            assert np.isin(rays["o"][m, b], planes[b]).all() and (rays["d"][m, b] == 0).all()
        m = axis == a
        seen |= {(a, float(s), bool(z1), bool(z2)) for s, z1, z2 in
                 zip(rays["d"][m, a], np.signbit(rays["d"][m, (a + 1) % 3]), np.signbit(rays["d"][m, (a + 2) % 3]))}
    assert len(seen) == 3 * 2 * 4  # every axis, both ways, both signs of each zero


def test_both_sides_of_each_threshold_occur(rubik_scene):
    orc = O.Oracle(rubik_scene)
    rays, labels, near = SR.epsilon_t(rubik_scene, with_near=True)
    m = np.char.startswith(labels, "epsilon_t/t_min")
    takes_near = orc.trace_closest(1, rays[m])[0] == near[m]
    assert takes_near.mean() >= 0.10 and (~takes_near).mean() >= 0.10  # t > 0.00001f accepts it / does not
    rays, labels, near = SR.parallel_threshold(rubik_scene, with_near=True)
    m = np.char.startswith(labels, "parallel_threshold/scale")
    takes_near = orc.trace_closest(1, rays[m])[0] == near[m]
    assert takes_near.mean() >= 0.10 and (~takes_near).mean() >= 0.10  # |a| >= 0.0001f / parallel
    # the scaled directions put float64's |a| within a few float32 ulp of the threshold
    a = np.abs(SR.mt_a(rubik_scene, near[m], rays["d"][m]))
    assert (np.abs(a / float(SR.A_MIN) - 1.0) < 1e-5).all()


def test_long_directions_reach_the_division_fallback_of_the_triangle_test(rubik_scene, families, traced):
    """parallel_threshold/huge_a: accepted triangles whose |a| >= 2^126, where the kernels' Newton reciprocal gives
    way to the division (traversal.hpp tri_prep), 1.0 / a is a denormal, and the accepted t is above 0.00001."""
    rays, labels = families["parallel_threshold"]
    tri, t, _ = traced["parallel_threshold"]
    m = (labels == "parallel_threshold/huge_a") & (tri != MISS)
    assert m.sum() >= 200
    a = np.abs(SR.mt_a(rubik_scene, tri[m], rays["d"][m]))
    assert (a >= SR.HUGE_A).all() and (a < 2.0 ** 128).all()
    assert (t[m] > SR.T_MIN).all() and (t[m] < 1e-3).all()


def test_special_values_cover_every_listed_special(families, traced):
    rays, labels = families["special_values"]
    tri, t, _ = traced["special_values"]
    assert (tri != MISS).mean() >= 0.10
    assert np.isnan(t).any()  # a NaN intersection_distance comes back as it went in
    bits = lambda x: np.asarray(x, np.float32).view(np.uint32)  # noqa: E731
    for field, specials in (("d", SR.D_SPECIALS), ("o", SR.O_SPECIALS)):
        for v in specials:
            for a in range(3):
                same = np.isnan(rays[field][:, a]) if np.isnan(v) else bits(rays[field][:, a]) == bits(v)
                assert same.any(), (field, a, v)
    for v in SR.T_SPECIALS:
        assert (np.isnan(rays["t"]) if np.isnan(v) else bits(rays["t"]) == bits(v)).any(), v
    assert (bits(rays["d"]) == 0).all(axis=1).any()  # the all-zero direction
    assert np.char.startswith(labels, "special_values/pair_").sum() >= 1000
    # the listed direction specials include values on recip_exact's division fallback: outside [2^-126, 2^126)
    m = np.abs(np.asarray(SR.D_SPECIALS, np.float64))
    assert ((m < 2.0 ** -126) & (m > 0)).any() and (m >= 2.0 ** 126).any() and (m == 2.0 ** -126).any()


def test_mixed_wave_interleaves_every_family_with_generic_rays(families):
    rays, labels = families["mixed_wave"]
    assert (labels[1::2] == "mixed_wave/generic").all()
    kinds = np.array([s.split("/")[1] for s in labels[0::2]])
    names = [f.__name__ for f in SR.FAMILIES]
    assert (kinds[: 2 * len(names)] == np.tile(names, 2)).all()  # round-robin: each wave of 64 holds every family
    for w in range(0, len(rays) - 63, 64):
        assert set(kinds[w // 2: w // 2 + 32]) == set(names)


def _decisions(scene, rays, dist, lo=np.fmin, hi=np.fmax, chunk=512):
    """(oracle accept, three-term accept) for every ray x node; dist: a scalar or one value per ray."""
    a, b = [], []
    for s in range(0, len(rays), chunk):
        r = rays[s:s + chunk]
        t0, t1 = SR.slab_terms(scene, r["o"], r["d"])
        tn, tf, ret = SR.intersects_box(t0, t1, lo, hi)
        d = dist if np.ndim(dist) == 0 else np.asarray(dist[s:s + chunk], np.float32)[:, None]
        a.append(SR.accept_oracle(ret, d))
        b.append(SR.accept_three_term(tn, tf, d))
    return np.concatenate(a), np.concatenate(b)


@pytest.mark.parametrize("name", ["on_plane_axis", "on_plane_one_zero"])
def test_three_term_box_test_is_intersects_box(rubik_scene, families, traced, name):
    """traversal.hpp box_test against IntersectsBox + `b < dist && !isinf(b)`: the root and every node."""
    rays, _ = families[name]
    t_hit = traced[name][1]
    f32 = np.float32
    total = 0
    for dist in (f32(1e30), f32(np.inf), f32(np.nan), f32(0), f32(-1), f32(-np.inf), f32(3.0), t_hit):
        want, got = _decisions(rubik_scene, rays, dist)
        assert (want == got).all(), dist
        total += int(want.sum())
    # and accepts are no rarity: a ray that hits accepted its root and a leaf, with dist = 1e30 and with dist = inf
    assert total >= 2 * 2 * 0.20 * len(rays)
    # 0 * inf: the NaN term loses to the other operand, which is the same axis' infinite term, so the box's entry or
    # exit is infinite and the node is rejected -- an origin on a box plane is outside that box for a ray along it
    nan_node = np.zeros(want.shape, bool)
    for s in range(0, len(rays), 512):
        t0, t1 = SR.slab_terms(rubik_scene, rays["o"][s:s + 512], rays["d"][s:s + 512])
        nan_node[s:s + 512] = (np.isnan(t0) | np.isnan(t1)).any(axis=2)
    want, _ = _decisions(rubik_scene, rays, f32(np.inf))
    assert nan_node.any(axis=1).all() and not want[nan_node].any()
    # a NaN tn comes with a NaN tf (each needs all three axes' terms NaN), so `tn <= tf` and `!(tn > tf)` agree
    # wherever b < dist can hold: the equivalence comment's "NaN bound" case never reaches the select
    t0, t1 = SR.slab_terms(rubik_scene, rays["o"][:256], rays["d"][:256])
    tn, tf, _ = SR.intersects_box(t0, t1)
    assert (np.isnan(tn) == np.isnan(tf)).all()


def test_two_record_frames_keep_on_plane_origins_on_plane(rubik_scene, families):
    """The world rays of the two-record scene of the GPU test, back in each record's model space."""
    for name in ("on_plane_axis", "on_plane_one_zero"):
        rays, _ = families[name]
        w = SR.world_for_translate(rays)
        o, d = SR.xform(SR.frame_translate(), w["o"], 1.0), SR.xform(SR.frame_translate(), w["d"], 0.0)
        zero_axis = rays["d"] == 0
        assert (o[zero_axis].view(np.uint32) == rays["o"][zero_axis].view(np.uint32)).all()  # exactly on the plane
        assert (d == rays["d"]).all()
        assert SR.nan_slab(rubik_scene, o, d).all()
        w = SR.world_for_permute(rays)
        o, d = SR.xform(SR.frame_permute(), w["o"], 1.0), SR.xform(SR.frame_permute(), w["d"], 0.0)
        assert (o == rays["o"]).all() and (d == rays["d"]).all()  # (a zero's sign may differ: the sums of zeros)
        assert SR.nan_slab(rubik_scene, o, d).all()
    # an infinite component turns the other rows' zero products into NaN
    rays, _ = families["special_values"]
    w = SR.world_for_permute(rays)
    inf_in = np.isinf(rays["o"]).any(axis=1)
    o = SR.xform(SR.frame_permute(), w["o"], 1.0)
    assert inf_in.any() and np.isnan(o[inf_in]).any(axis=1).all()
