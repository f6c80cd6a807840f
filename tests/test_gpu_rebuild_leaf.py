"""GPU: the device rebuild with leaves of several triangles (include/srt_rebuild_leaf.h, Query.set_rebuild_leaf) against
the host mirror srt_bvh_build_lbvh_leaf -- the tree walked from the root, every box and .w dword, the pair numbering -- and
against the CPU oracle on the host-built arrays, the oracle's hit position mapped through the order.

tests/test_rebuild_leaf_api.py holds the mirror to a numpy restatement of the rule.  Scenes of tests/rebuild_ref.py: Rubik;
the lifted 24 x 24 quad grid; 64 copies of one triangle (every key equal); three triangles (max_leaf 2: a leaf of one and
a leaf of two; max_leaf 4: a leaf root); one triangle (a leaf root); a mesh with two vertex indices out of range.  And
511 copies of one triangle at max_leaf 255 (tests/scale_scenes.py): a leaf of 255, the largest count there is.
"""
import numpy as np
import pytest

import rebuild_leaf_ref as LR
import rebuild_ref as BR
import refit_ref as RR
import scale_scenes as SC
import srt_amd as S
from conftest import OBJECTS, bits_equal
from oracle import pyoracle as O
from test_gpu_queries import MISS, bounds, sphere_rays, to_dev
from test_gpu_rebuild import check_hits, expected_schedule, scene_rays, verts_dev

pytestmark = pytest.mark.gpu

NAMES = ("rubik", "grid", "copies", "three", "one", "oob")
LEAVES = (2, 4, 8)


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


@pytest.fixture(scope="module")
def rubik():
    return S.load_obj(OBJECTS / "Rubik" / "Rubik.obj")


class Cases:
    """(scene, verts, host-built scene, order, rays, the oracle's answer on the host-built scene) per scene and
    max_leaf, made on first use and kept: the oracle traces each tree once."""

    def __init__(self, rubik):
        self.rubik, self.scenes, self.made = rubik, {}, {}

    def __call__(self, name, max_leaf):
        if name not in self.scenes:
            self.scenes[name] = BR.make_scene(name, self.rubik)
        if (name, max_leaf) not in self.made:
            scene, verts = self.scenes[name]
            built, order = S.build_lbvh(scene, verts, max_leaf=max_leaf)
            rays = scene_rays(name, built)
            self.made[name, max_leaf] = (scene, verts, built, order, rays, O.Oracle(built).trace_closest(1, rays))
        return self.made[name, max_leaf]


@pytest.fixture(scope="module")
def cases(rubik):
    return Cases(rubik)


def pairs_loop(nodes):
    """The uint32 [4 m, 4] pair rows a mirror-built node array stands for, pair by pair: pair r holds nodes 2r + 1 and
    2r + 2 (tests/scale_scenes.py pairs_from_nodes is the same without the loop, held equal on the CPU)."""
    m = (len(nodes) - 1) // 2
    want = np.zeros((4 * m, 4), np.uint32)  # the .w dwords by pair number
    for r in range(m):
        for slot in (0, 1):
            node = nodes[2 * r + 1 + slot]
            count = int(node["count"])
            want[4 * r + 2 * slot, 3] = int(node["first"]) if count else (int(node["first"]) - 1) // 2
            want[4 * r + 2 * slot + 1, 3] = count
            want[4 * r + 2 * slot, :3] = node["min"].view(np.uint32)
            want[4 * r + 2 * slot + 1, :3] = node["max"].view(np.uint32)
    return want


def check_structure(q, built, order):
    """The device layout against the mirror's node array: the walk from the root (leaf or not, first triangle, count,
    the six box dwords), the pair numbering (pair r holds nodes 2r + 1 and 2r + 2), the pair rows the object reports,
    the triangle records and the order."""
    pairs, roots, tris = q.layout()
    BR.assert_same_tree(BR.walk_layout(pairs, roots), BR.walk_nodes(built.nodes))
    assert (roots[2:4] == roots[0:2]).all()  # the ghost root is the root
    m = (len(built.nodes) - 1) // 2
    assert pairs.shape == (4 * max(m, 1), 4)
    want = pairs_loop(built.nodes)
    assert (pairs[:4 * m] == want).all(), f"{(pairs[:4 * m] != want).sum()} pair dwords differ"
    assert (tris == BR.layout_tris(built)).all(), f"{(tris != BR.layout_tris(built)).sum()} tris dwords differ"
    assert (q.tri_order() == order).all()


def check_counters(q, scene, built, max_leaf):
    m, largest, depth = LR.shape(built.nodes)
    n = len(scene.tris)
    heights, launches = expected_schedule(built)
    assert heights == depth
    assert q.get_int("rebuild.leaf") == max_leaf
    assert q.get_int("rebuild.pairs") == m and q.get_int("layout.pairs") == 64 * max(m, 1)
    assert q.get_int("rebuild.max_leaf") == largest and q.get_int("rebuild.depth") == depth
    assert q.get_int("stack.entries") == depth + 1 and q.get_int("stack.packed") == 1
    assert q.get_int("stack.in_hbm") == (1 if 256 * 3 * 4 * (depth + 1) > 65536 else 0)
    assert q.get_int("refit.heights") == heights and q.get_int("refit.launches") == launches
    # its own launches: a refit alone (one triangle); box, box, keys, sort, permute, root (a leaf root); those four, then
    # range, scan, emit, permute, climb, schedule (max_leaf > 1); srt_rebuild.h's eight (max_leaf == 1)
    own = 0 if n == 1 else (6 if n <= max_leaf else (10 if max_leaf > 1 else 8))
    assert q.get_int("rebuild.launches") == own + launches


@pytest.mark.parametrize("max_leaf", LEAVES)
@pytest.mark.parametrize("name", NAMES)
def test_structure_hits_and_counters_after_a_collapsed_rebuild(torch, cases, name, max_leaf):
    """set_rebuild_leaf, the rebuild, closest and occluded enqueued back to back on a non-default stream."""
    from srt_amd.query import Query

    scene, verts, built, order, rays, oracle = cases(name, max_leaf)
    stream = torch.cuda.Stream()
    with Query(scene, stream=stream, refit=True, rebuild=True) as q:
        assert q.get_int("rebuild.leaf") == 1 and q.get_int("rebuild.leaf_bytes") == 0
        assert q.get_int("rebuild.pairs") == 0 and q.get_int("rebuild.max_leaf") == 0
        bytes_before = q.get_int("rebuild.bytes")
        q.set_rebuild_leaf(max_leaf)
        assert q.get_int("rebuild.bytes") == bytes_before and q.get_int("rebuild.count") == 0
        assert (q.get_int("rebuild.leaf_bytes") > 0) == (len(scene.tris) > 1)
        with torch.cuda.stream(stream):
            v = verts_dev(torch, verts)
            dev = to_dev(torch, rays)
            q.rebuild(v)
            hits = q.closest(dev)
            occ = q.occluded(dev)
        stream.synchronize()
        hits, occ = hits.numpy(), occ.cpu().numpy()
        check_structure(q, built, order)
        check_counters(q, scene, built, max_leaf)
        assert q.get_int("rebuild.count") == 1
    if name == "three":
        counts = sorted(int(c) for c in built.nodes["count"])
        assert counts == ([0, 1, 2] if max_leaf == 2 else [3])  # a 1-leaf and a 2-leaf; a leaf root
    if name == "one":
        assert len(built.nodes) == 1
    hit = check_hits(built, order, hits, oracle)
    assert (occ == hit).all()
    assert hit.sum() >= 100, "the rays must find the mesh"


def test_a_leaf_of_255_keeps_packed_stack_entries(torch):
    """The largest max_leaf there is: 511 copies of one triangle (every key equal, so the positions decide: the root
    splits [0, 255] from [256, 510], and the right side is one leaf of 255 -- tests/test_scale_scenes.py holds the mirror
    to that).  A count of 255 still fits the packed stack entry (csrc/query_host.cpp: max_leaf < 256)."""
    from srt_amd import SrtError, _lib
    from srt_amd.query import Query

    scene, verts = SC.leaf255_scene()
    built, order = S.build_lbvh(scene, verts, max_leaf=255)
    assert len(scene.tris) == 511 and sorted(int(c) for c in built.nodes["count"]) == [0, 0, 128, 128, 255]
    rays = scene_rays("copies", built)  # from outside the box and aimed at the copies
    oracle = O.Oracle(built).trace_closest(1, rays)
    stream = torch.cuda.Stream()
    with Query(scene, stream=stream, refit=True, rebuild=True) as q:
        with pytest.raises(SrtError) as e:
            q.set_rebuild_leaf(256)
        assert e.value.code == _lib.SRT_ERR_INVALID and "[1, 255]" in str(e.value)
        del e
        assert q.get_int("rebuild.leaf") == 1
        q.set_rebuild_leaf(255)
        assert q.get_int("rebuild.leaf") == 255
        with torch.cuda.stream(stream):
            v = verts_dev(torch, verts)
            dev = to_dev(torch, rays)
            q.rebuild(v)
            hits = q.closest(dev)
            occ = q.occluded(dev)
        stream.synchronize()
        hits, occ = hits.numpy(), occ.cpu().numpy()
        assert q.get_int("rebuild.max_leaf") == 255 and q.get_int("stack.packed") == 1
        check_structure(q, built, order)
        check_counters(q, scene, built, 255)
        assert q.get_int("rebuild.count") == 1
    hit = check_hits(built, order, hits, oracle)
    assert (occ == hit).all()
    assert hit.sum() >= 100, "the rays must find the mesh"


BOTH_WAYS = ((4, 1), (1, 4))


@pytest.mark.parametrize("name,changes", [
    pytest.param("rubik", BOTH_WAYS, id="rubik"), pytest.param("grid", BOTH_WAYS, id="grid"),
    pytest.param("copies", BOTH_WAYS, id="copies"), pytest.param("three", BOTH_WAYS, id="three"),
    # a collapsed tree of m > 0 pairs, then a leaf root: no emit kernel runs, so nothing the first rebuild read back
    # (its m, its largest leaf) may reach the second tree
    pytest.param("three", ((2, 4),), id="three-2-then-4")])
def test_no_state_is_carried_between_max_leaf_values(torch, cases, name, changes):
    """max_leaf 4 then 1 gives the dwords of a fresh max_leaf 1 object, and 1 then 4 those of a fresh max_leaf 4 one."""
    from srt_amd.query import Query

    keys = ("stack.entries", "stack.in_hbm", "stack.packed", "refit.heights", "refit.launches", "refit.bytes", "rebuild.depth",
            "rebuild.launches", "rebuild.pairs", "rebuild.max_leaf", "rebuild.leaf", "layout.pairs", "layout.roots",
            "layout.tris", "scene.bytes")
    for first, second in changes:
        scene, verts, built, order, rays, oracle = cases(name, second)
        with Query(scene, refit=True, rebuild=True, rebuild_leaf=first) as q, \
                Query(scene, refit=True, rebuild=True, rebuild_leaf=second) as once:
            q.rebuild(verts_dev(torch, RR.wave(scene.verts, 1.5, 0.7)))  # other vertices: another order
            assert q.get_int("rebuild.leaf") == first
            q.set_rebuild_leaf(second)
            q.rebuild(verts_dev(torch, verts))
            once.rebuild(verts)  # the numpy path uploads and synchronises
            for g, w in zip(q.layout(), once.layout()):
                assert g.shape == w.shape and (g == w).all(), (first, second)
            assert (q.tri_order() == once.tri_order()).all()
            check_structure(q, built, order)
            check_counters(q, scene, built, second)
            assert q.get_int("rebuild.count") == 2 and once.get_int("rebuild.count") == 1
            for key in keys:
                assert q.get_int(key) == once.get_int(key), (key, first, second)
            if second == 1:  # what tests/test_gpu_rebuild.py pins for an object that never saw the setting
                assert q.get_int("rebuild.launches") == 8 + expected_schedule(built)[1]
                assert q.get_int("layout.pairs") == 64 * (len(scene.tris) - 1)
            check_hits(built, order, q.closest(to_dev(torch, rays)).numpy(), oracle)


@pytest.mark.parametrize("name", ["rubik", "grid", "copies", "three", "oob"])
def test_collapsed_rebuild_then_refit_keeps_the_topology(torch, cases, name):
    from srt_amd.query import Query

    scene, verts, built, order, rays, _ = cases(name, 4)
    other = RR.wave(verts, 0.4, 1.1)
    want = S.refit_scene(built, other)  # the collapsed topology, srt_bvh_refit with the refit's vertices
    with Query(scene, refit=True, rebuild=True, rebuild_leaf=4) as q:
        q.rebuild(verts_dev(torch, verts))
        q.refit(verts_dev(torch, other))
        hits = q.closest(to_dev(torch, rays)).numpy()
        check_structure(q, want, order)
        check_counters(q, scene, want, 4)
        assert q.get_int("rebuild.count") == 1 and q.get_int("refit.count") == 1
    check_hits(want, order, hits, O.Oracle(want).trace_closest(1, rays))


def test_surface_and_temporal_objects_stay_valid(torch, cases):
    """srt_hit.triangle stays the scene's triangle index after a collapsed rebuild: a Surface and a Temporal object built
    from the scene give, on the rebuilt query's hits, bit for bit what they give on the hits of a query that was only
    refit to the same vertices.  Rays that hit two triangles at one distance are dropped on the CPU."""
    from srt_amd.query import Query
    from srt_amd.surface import Surface
    from srt_amd.temporal import Temporal

    scene, verts, _, _, _, _ = cases("rubik", 4)
    W, H = 64, 63
    frames = [verts, RR.wave(scene.verts, 0.3, 0.9)]
    lo, hi = bounds(S.refit_scene(scene, verts))
    rays = sphere_rays(lo, hi, 4099, 404)
    keep = np.ones(len(rays), bool)
    for v in frames:  # the oracle alone: where the two trees name different triangles, two lie at one distance
        b, o = S.build_lbvh(scene, v, max_leaf=4)
        tri_b, t_b, _, _ = O.Oracle(b).trace_closest(1, rays)
        tri_r, t_r, _, _ = O.Oracle(S.refit_scene(scene, v)).trace_closest(1, rays)
        assert bits_equal(t_b, t_r).all()
        keep &= np.where(tri_b != MISS, o[np.where(tri_b != MISS, tri_b, 0)], MISS) == tri_r
    assert (~keep).mean() <= 0.01
    rays = rays[keep][:W * H]
    assert len(rays) == W * H
    cam = ((0.0, 0.0, 30.0), (0.0, 0.0, -1.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0))
    rng = np.random.default_rng(5)
    dev = to_dev(torch, rays)
    with Query(scene, refit=True, rebuild=True, rebuild_leaf=4) as qb, Query(scene, refit=True) as qr, \
            Surface(scene, refit=True) as surf, Temporal(W, H) as tb, Temporal(W, H) as tr:
        tb.set_mesh(scene)
        tr.set_mesh(scene)
        for k, v in enumerate(frames):
            vd = verts_dev(torch, v)
            qb.rebuild(vd)
            qr.refit(vd)
            surf.refit(vd)
            assert qb.get_int("rebuild.max_leaf") > 1
            hb, hr = qb.closest(dev), qr.closest(dev)
            assert (hb.raw == hr.raw).all() and 0.25 < float(hb.hit.float().mean()) < 0.95
            assert (surf.shade(dev, hb) == surf.shade(dev, hr)).all()
            acc = np.ones((H, W, 4), np.float32)
            acc[..., :3] = rng.uniform(0, 6, (H, W, 3)).astype(np.float32)
            acc = torch.from_numpy(acc).cuda()
            tb.set_vertices(vd)
            tr.set_vertices(vd)
            a, b = tb.accumulate(acc, 3, hb, cam), tr.accumulate(acc, 3, hr, cam)
            assert (a.view(torch.int32) == b.view(torch.int32)).all(), f"frame {k}"


def test_argument_errors_enqueue_nothing(torch, cases):
    from srt_amd import SrtError, _lib
    from srt_amd.query import Query

    scene, verts, built, order, rays, oracle = cases("rubik", 4)
    rays = rays[:1500]
    good = verts_dev(torch, verts)

    def invalid(call, text):
        with pytest.raises(SrtError) as e:
            call()
        assert e.value.code == _lib.SRT_ERR_INVALID and text in str(e.value)

    with Query(scene) as plain, Query(scene, refit=True) as flagged:
        for q in (plain, flagged):
            invalid(lambda: q.set_rebuild_leaf(4), "not enabled")
            assert q.get_int("rebuild.leaf") == 0 and q.get_int("rebuild.leaf_bytes") == 0
            assert q.get_int("rebuild.pairs") == 0 and q.get_int("rebuild.max_leaf") == 0
    with pytest.raises(SrtError):
        Query(scene, refit=True, rebuild=True, rebuild_leaf=0)
    with Query(scene, refit=True, rebuild=True) as q:
        q.set_rebuild_leaf(4)
        q.rebuild(good)
        before, hits_before = q.layout(), q.closest(to_dev(torch, rays)).numpy()
        state = [q.get_int(k) for k in ("rebuild.leaf", "rebuild.count", "rebuild.launches", "rebuild.pairs", "rebuild.max_leaf",
                                        "rebuild.bytes", "rebuild.leaf_bytes", "layout.pairs", "stack.entries")]
        for bad in (0, 256, 1000, 0xFFFFFFFF):
            invalid(lambda: q.set_rebuild_leaf(bad), "[1, 255]")
        with pytest.raises(ValueError):
            q.set_rebuild_leaf(-1)
        assert [q.get_int(k) for k in ("rebuild.leaf", "rebuild.count", "rebuild.launches", "rebuild.pairs", "rebuild.max_leaf",
                                       "rebuild.bytes", "rebuild.leaf_bytes", "layout.pairs", "stack.entries")] == state
        for g, w in zip(q.layout(), before):
            assert g.shape == w.shape and (g == w).all()
        hits = q.closest(to_dev(torch, rays)).numpy()
        assert hits.tobytes() == hits_before.tobytes()
        # a good value after the bad ones takes effect at the next rebuild only
        q.set_rebuild_leaf(8)
        assert q.get_int("rebuild.leaf") == 8 and q.get_int("rebuild.max_leaf") == state[4]
        for g, w in zip(q.layout(), before):
            assert (g == w).all()
        q.set_rebuild_leaf(4)
        q.rebuild(good)
        check_structure(q, built, order)
