"""GPU: ray traversal at special values -- origins on box planes, axis-parallel and zero direction components, hits
at the 0.00001 and 0.0001 thresholds, infinities, NaNs, denormals and huge values -- against the CPU oracle, bit for
bit, through Query.closest, Query.occluded and Compute.trace_closest.

The ray sets are tests/special_rays.py's; tests/test_special_rays_cpu.py checks with the oracle alone that they reach
what they are named for (run it first when something fails here: it also holds box_test's algebra to IntersectsBox
in numpy, which tells an algebra fault from an instruction-selection one).  Each scene is the smallest that selects
its code path, and the path is asserted through get_int.
"""
import numpy as np
import pytest

import refit_ref as RR
import special_rays as SR
import srt_amd as S
from conftest import OBJECTS, bits_equal
from oracle import pyoracle as O
from test_gpu_queries import MISS, _deep_chain, check_closest, to_dev
from test_gpu_refit import verts_dev

pytestmark = pytest.mark.gpu

SCENES = ("rubik", "deep_chain", "big_leaf", "two_rubiks", "rubik_refit")


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


def same_centroid_leaf(n=256):
    """test_gpu_refit.same_centroid_triangles extended to n triangles: every triangle's corners sum to exactly zero,
    so all centroids coincide, no split separates them, and the root is one leaf of n triangles."""
    tri = []
    for k in range(n):
        a, b = np.array([k + 1.0, 0.5 * k, -1.0]), np.array([-2.0, k + 2.0, 0.25 * k])
        tri.append([a, b, -(a + b)])
    return np.asarray(tri, np.float32).reshape(-1, 9)


class Case:
    """One scene with its rays: `scene` is what the oracle (and a fresh Compute) traces; `base` what the Query object
    is created from (differs for the refit case, which then moves to `verts`)."""

    def __init__(self, scene, sets, bvh_count=1, base=None, verts=None, n0=None):
        self.scene, self.bvh_count, self.base, self.verts, self.n0 = scene, bvh_count, base or scene, verts, n0
        self.rays, self.labels = SR.concat(list(sets.values()))
        self.tri, self.t, _, st = O.Oracle(scene).trace_closest(bvh_count, self.rays)
        assert st["stack_overflow"] == 0

    def bvh_of(self):
        return None if self.n0 is None else (lambda tri: (tri >= self.n0).astype(np.uint32))

    def query(self, stream=None):
        from srt_amd.query import Query

        return Query(self.base, stream=stream, refit=self.verts is not None)


def build_case(name):
    rubik = S.load_obj(OBJECTS / "Rubik" / "Rubik.obj")
    if name == "rubik":
        scene = S.Scene.from_models([rubik])
        return Case(scene, SR.all_families(scene))
    if name == "deep_chain":
        scene = S.Scene.from_models([S.model_from_triangles(_deep_chain(), kd=(0.6, 0.6, 0.6), ks=(0.1, 0.1, 0.1), ns=8.0)])
        return Case(scene, SR.all_families(scene))  # from its own planes
    if name == "big_leaf":
        scene = S.Scene.from_models([S.model_from_triangles(same_centroid_leaf())])
        assert len(scene.nodes) == 1 and scene.nodes["count"][0] == 256
        return Case(scene, SR.all_families(scene))  # its only planes are the root's
    if name == "two_rubiks":
        # record 0: translated by amounts that keep on-plane origins on-plane; record 1: axes permuted, one negated;
        # bvh_count = 3 brings in the zero record past the array.  The model-space rays alternate between the frames.
        one = S.Scene.from_models([rubik])
        scene = S.Scene.from_models([rubik, S.load_obj(OBJECTS / "Rubik" / "Rubik.obj")])
        scene.bvhs[0]["frame"], scene.bvhs[1]["frame"] = SR.frame_translate(), SR.frame_permute()
        sets = {}
        for fam, (rays, labels) in SR.all_families(one).items():
            w = SR.world_for_translate(rays)
            w[1::2] = SR.world_for_permute(rays)[1::2]
            sets[fam] = (w, labels)
        return Case(scene, sets, bvh_count=3, n0=len(one.tris))
    assert name == "rubik_refit"
    base = S.Scene.from_models([rubik])
    verts = RR.wave(base.verts)
    scene = S.refit_scene(base, verts)
    return Case(scene, SR.all_families(scene), base=base, verts=verts)  # from the refit scene's planes


@pytest.fixture(scope="module")
def cases():
    """Built on first use and kept: the rays and the oracle's answers are computed once per scene."""
    made = {}

    def get(name):
        if name not in made:
            made[name] = build_case(name)
        return made[name]

    return get


def families_of(labels, bad):
    names, counts = np.unique(labels[bad], return_counts=True)
    return ", ".join(f"{n}: {c}" for n, c in zip(names, counts))


def assert_path(q, name):
    if name in ("rubik", "two_rubiks", "rubik_refit"):
        assert q.get_int("stack.in_hbm") == 0 and q.get_int("stack.packed") == 1  # LDS stacks, packed entries
    elif name == "deep_chain":
        assert q.get_int("stack.in_hbm") == 1  # stacks in HBM
    else:
        assert q.get_int("stack.packed") == 0  # a leaf of 256 triangles: unpacked entries, hundreds of leaf steps


def run_query(torch, case, name, rays):
    with case.query() as q:
        q.set_bvh_count(case.bvh_count)
        if case.verts is not None:
            q.refit(verts_dev(torch, case.verts))
        assert_path(q, name)
        dev = to_dev(torch, rays)
        hits = q.closest(dev).numpy()
        occ = q.occluded(dev).cpu().numpy()
        refill = q.get_int("refill.min")
    return hits, occ, refill


def assert_matches(case, rays, labels, tri_o, t_o, hits, occ):
    bad = (hits["triangle"] != tri_o) | ~bits_equal(hits["t"], t_o)
    assert not bad.any(), f"closest differs from the oracle in {bad.sum()} rays ({families_of(labels, bad)})"
    bad = occ != (tri_o != MISS)
    assert not bad.any(), f"occluded differs from the oracle in {bad.sum()} rays ({families_of(labels, bad)})"
    check_closest(case.scene, case.bvh_count, rays, hits, bvh_of=case.bvh_of())  # every field, and the miss record


@pytest.mark.parametrize("name", SCENES)
def test_query_closest_and_occluded(torch, cases, name):
    case = cases(name)
    hits, occ, refill = run_query(torch, case, name, case.rays)
    assert refill == 48  # SRT_QUERY_REFILL at its default for these scenes
    assert_matches(case, case.rays, case.labels, case.tri, case.t, hits, occ)


@pytest.mark.parametrize("name", SCENES)
def test_compute_trace_closest(cases, name):
    """The path tracer's closest-hit kernel: box_t / box_ok / tri_accept / recip_normal."""
    case = cases(name)
    c = S.Compute().Init()
    try:
        c.bind_scene(case.scene)
        c.SetUInt("bvh_count", case.bvh_count)
        hits, t = c.trace_closest(case.rays)
    finally:
        c.close()
    bad = (hits != case.tri) | ~bits_equal(t, case.t)
    assert not bad.any(), f"trace_closest differs from the oracle in {bad.sum()} rays ({families_of(case.labels, bad)})"


@pytest.mark.parametrize("n", [1, 63, 65])
def test_ray_counts_around_one_wave(torch, cases, n):
    """mixed_wave's first rays (every family beside generic rays) in less than, and just over, one 64-lane wave."""
    case = cases("rubik")
    m = np.flatnonzero(SR.family_of(case.labels) == "mixed_wave")[:n]
    if n == 1:
        m = np.flatnonzero(case.labels == "mixed_wave/special_values")[:1]
    rays, labels = case.rays[m].copy(), case.labels[m]
    hits, occ, _ = run_query(torch, case, "rubik", rays)
    assert_matches(case, rays, labels, case.tri[m], case.t[m], hits, occ)


@pytest.mark.parametrize("refill", [1, 64])
def test_refill_thresholds(torch, cases, monkeypatch, refill):
    """SRT_QUERY_REFILL is read when the object is created: 1 repacks lanes only when a whole wave is done, 64
    whenever one lane is."""
    monkeypatch.setenv("SRT_QUERY_REFILL", str(refill))
    case = cases("rubik")
    hits, occ, got = run_query(torch, case, "rubik", case.rays)
    assert got == refill
    assert_matches(case, case.rays, case.labels, case.tri, case.t, hits, occ)
