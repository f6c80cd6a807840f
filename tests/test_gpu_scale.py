"""GPU: the device refit and rebuild past one block and one sort tile, on the scenes of tests/scale_scenes.py, with the
comparisons of the small tests: the host mirrors dword for dword and the CPU oracle bit for bit.

What each scene crosses (tests/test_scale_scenes.py holds the scenes to it on the CPU, and every test here asserts its
own regime again, so a scene shrunk later fails instead of passing vacuously):
  knot70k (69,632 triangles)  box_partial_kernel's grid-stride loop and all 256 partial boxes; the radix sort's merge path
      over 272 blocks; the exclusive scan over many tiles; climb / schedule / emit with 272 blocks sharing the counts,
      cursors and arrival words; three and more refit launches of a height of their own; a rebuilt tree deep enough to
      move the stacks from LDS to HBM; the path tracer's own choice of global-scene mode, triangle slots and a top region;
  clusters  17 keys of 4,096 triangles each, every key in every block of the sort: the order among equal keys;
  knot70k_and_rubik  the 64-bit (record, key) sort on the merge path, seg_box_kernel's one-owner path 272 times;
  knot70k_and_rubik_shuffled  the same two records interleaved leaf by leaf: mixed-owner blocks throughout, owners that
      cross every tile of the sort, and the hit remap over an order that is no concatenation of two runs;
  soup1m (1,052,672 triangles)  onesweep.
Python walks of the tree are used up to 70 k triangles, beside scale_scenes.pairs_from_nodes; at 1 M the vectorised
forms alone.
"""
import dataclasses

import numpy as np
import pytest

import rebuild_leaf_ref as LR
import rebuild_models_ref as MR
import rebuild_ref as BR
import refit_ref as RR
import scale_scenes as SC
import special_rays as SR
import srt_amd as S
import test_gpu_rebuild_leaf as LT
import test_gpu_rebuild_models as MT
from conftest import OBJECTS, bits_equal
from oracle import pyoracle as O
from srt_amd import render as R
from test_gpu_queries import MISS, check_closest, sphere_rays, to_dev
from test_gpu_rebuild import check_hits, expected_schedule, scene_rays, verts_dev
from test_gpu_refit import assert_layouts_equal
from test_gpu_scene_refit import assert_arrays_equal, expected_tri_slots

pytestmark = pytest.mark.gpu

STATE_KEYS = ("stack.entries", "stack.in_hbm", "stack.packed", "refit.heights", "refit.launches", "refit.bytes", "rebuild.depth",
              "rebuild.launches", "rebuild.pairs", "rebuild.max_leaf", "rebuild.leaf", "layout.pairs", "layout.roots",
              "layout.tris", "scene.bytes")  # test_gpu_rebuild_leaf.test_no_state_is_carried_between_max_leaf_values'
LAYOUT_ENV = ("SRT_FORCE_GLOBAL_SCENE", "SRT_TRI_ALIGN", "SRT_TOP_DEPTH", "SRT_NODE_ALIGN", "SRT_NODE_LAYOUT", "SRT_TREELETS",
              "SRT_TREELET_DEPTH", "SRT_GLOBAL_FUSED_MODE", "SRT_GLOBAL_WAVES_MODE")


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


@pytest.fixture(scope="module")
def rubik():
    return S.load_obj(OBJECTS / "Rubik" / "Rubik.obj")


class Cases:
    """Per scene (scene, verts), and per scene and max_leaf (scene, verts, mirror-built scene, order, rays, the oracle's
    answer on the mirror's arrays): made on first use and kept, so the mirror builds and the oracle traces each tree once."""

    def __init__(self, rubik):
        self.rubik, self.scenes, self.made = rubik, {}, {}

    def scene(self, name):
        if name not in self.scenes:
            self.scenes[name] = SC.make_scene(name, self.rubik)
        return self.scenes[name]

    def __call__(self, name, max_leaf):
        if (name, max_leaf) not in self.made:
            scene, verts = self.scene(name)
            records = len(scene.bvhs)
            if records > 1:
                built, order = S.build_lbvh_models(scene, verts, max_leaf=max_leaf)
                rays = MR.scene_rays(scene, verts)
            else:
                built, order = S.build_lbvh(scene, verts, max_leaf=max_leaf)
                if name == "soup1m":  # 1,000 rays: from outside the box (the mirror's root) and aimed at triangles
                    lo, hi = built.nodes[0]["min"].astype(np.float64), built.nodes[0]["max"].astype(np.float64)
                    rays = np.concatenate([sphere_rays(lo, hi, 700, 11), SR.triangle_rays(built, 300, 12)])
                else:
                    rays = scene_rays(name, built)  # the generic sets: 1,500 sphere rays and 600 triangle-aimed ones
            self.made[name, max_leaf] = (scene, verts, built, order, rays, O.Oracle(built).trace_closest(records, rays))
        return self.made[name, max_leaf]


@pytest.fixture(scope="module")
def cases(rubik):
    return Cases(rubik)


def check_structure(q, built, order, walk):
    """The device layout of a one-record object against the mirror's node array, vectorised: every dword of the pair rows
    (pair r holds nodes 2r + 1 and 2r + 2), of the root and the ghost root, of the triangle records; the order; and that the
    rows are a tree over every position.  With `walk` also the Python walk from the root of the small tests."""
    pairs, roots, tris = q.layout()
    n, m = len(built.tris), (len(built.nodes) - 1) // 2
    assert pairs.shape == (4 * max(m, 1), 4) and roots.shape == (4, 4)
    want = SC.pairs_from_nodes(built.nodes)
    assert (pairs[:4 * m] == want).all(), f"{(pairs[:4 * m] != want).sum()} pair dwords differ"
    assert (roots[0:2] == SC.root_from_nodes(built.nodes)).all()
    assert (roots[2:4] == roots[0:2]).all()  # the ghost root is the root
    SC.assert_is_a_tree(pairs, m, n)
    want = BR.layout_tris(built)
    assert tris.shape == want.shape and (tris == want).all(), f"{(tris != want).sum()} tris dwords differ"
    got = q.tri_order()
    assert (got == order).all(), f"{(got != order).sum()} positions differ"
    if walk:
        BR.assert_same_tree(BR.walk_layout(pairs, roots), BR.walk_nodes(built.nodes))


def as_values(rows):
    return rows.view(np.float32)[:, :3]


# -- a. Query.refit ----------------------------------------------------------------------------------------------------
def test_query_refit_at_scale(torch, cases):
    """refit, closest and occluded back to back on a non-default stream; then a refit back to the creation vertices."""
    from srt_amd.query import Query

    scene, verts = cases.scene("knot70k")
    assert len(scene.tris) == SC.N_KNOT > SC.box_loop_threshold()
    counts = RR.pair_height_counts(scene)
    assert (counts > SC.LEVEL).sum() >= 3  # three heights or more get a launch of their own
    heights, launches = expected_schedule(scene)
    want = S.refit_scene(scene, verts)
    rays = scene_rays("knot70k", want)
    stream = torch.cuda.Stream()
    with Query(scene, stream=stream, refit=True) as q, Query(want) as fresh:
        q.set_bvh_count(1)
        before = q.layout()
        assert q.get_int("refit.heights") == heights == len(counts)
        assert q.get_int("refit.launches") == launches and launches >= 2 + 3
        with torch.cuda.stream(stream):
            v = verts_dev(torch, verts)
            dev = to_dev(torch, rays)
            q.refit(v)
            hits = q.closest(dev)
            occ = q.occluded(dev)
        stream.synchronize()
        hits, occ = hits.numpy(), occ.cpu().numpy()
        got = q.layout()
        assert_layouts_equal(got, fresh.layout())
        assert not (got[0] == before[0]).all() and not (got[2] == before[2]).all()  # and it is no no-op
        with torch.cuda.stream(stream):
            q.refit(verts_dev(torch, scene.verts))
        stream.synchronize()
        assert q.get_int("refit.count") == 2
        back = q.layout()
        # the creation layout again: the builder's boxes as values (a zero's sign may differ), the rest in bits
        for g, w in zip(back[:2], before[:2]):
            assert g.shape == w.shape and (as_values(g) == as_values(w)).all() and (g[:, 3] == w[:, 3]).all()
        assert (back[2] == before[2]).all()
    tri_o, _ = check_closest(want, 1, rays, hits)
    hit = tri_o != MISS
    assert (occ == hit).all()
    assert hit.sum() >= 100, "the rays must find the mesh"


# -- b. Compute.refit --------------------------------------------------------------------------------------------------
def test_compute_refit_at_scale(torch, cases, monkeypatch):
    """The path tracer's own scene, laid out as the policy itself chooses for a scene of 1 MB or more (no environment
    override): bind(refit=True) and a device refit against a fresh bind of the host-refit scene -- every dword, a 64 x 40
    render at 2 spp, and trace_closest against the oracle."""
    for name in LAYOUT_ENV:
        monkeypatch.delenv(name, raising=False)
    scene, verts = cases.scene("knot70k")
    n = len(scene.tris)
    assert n == SC.N_KNOT and 32 * len(scene.nodes) + 48 * n >= 1 << 20
    want = S.refit_scene(scene, verts)
    rays = scene_rays("knot70k", want)
    tri_o, t_o, _, st = O.Oracle(want).trace_closest(1, rays)
    assert st["stack_overflow"] == 0 and (tri_o != MISS).sum() >= 100
    setup = dataclasses.replace(R.make_setup(64, 40, show_model=True, models=[R.torus_knot_model(272, 128)]), scene=scene)
    ra, rb = R.Renderer(setup), None
    try:
        a = ra.compute
        a.bind_scene(scene, refit=True)
        # the policy's own choice: triangle slots with gaps, fused sub-steps at 5 waves per SIMD, a top region
        assert a.GetInt("scene.tri_slots") == expected_tri_slots(scene) > n
        assert (a.GetInt("scene.fused"), a.GetInt("scene.global_waves")) == (1, 5)
        assert a.GetInt("scene.top_depth") > 0 and a.GetInt("scene.top_f4") > 0
        assert a.refit_get_int("refit.launches") >= 2 + 3 and a.refit_get_int("refit.treelets") == 0
        before = a.scene_device()
        a.refit(verts_dev(torch, verts))
        ra.render(2)  # nothing between the refit and the launches
        img, out = ra.accum().copy(), ra.output().copy()
        assert a.refit_get_int("refit.count") == 1
        # global-scene mode, the 5-wave fused instance with its LDS copy of the top levels
        assert (a.GetInt("launch.block"), a.GetInt("launch.blocks_per_cu")) == (256, 5)
        assert a.GetInt("launch.top_f4") == a.GetInt("scene.top_f4")
        got = a.scene_device()
        tri, t = a.trace_closest(rays)
        rb = R.Renderer(dataclasses.replace(setup, scene=want))  # the host path: a fresh upload of the host-refit scene
        b = rb.compute
        assert b.GetInt("scene.tri_slots") == a.GetInt("scene.tri_slots")
        assert_arrays_equal(got, b.scene_device())
        assert not (got[0] == before[0]).all() and not (got[2] == before[2]).all()
        rb.render(2)
        ref, ref_out = rb.accum().copy(), rb.output().copy()
    finally:
        ra.close()
        if rb is not None:
            rb.close()
    assert bits_equal(img, ref).all() and out.tobytes() == ref_out.tobytes()
    assert (ref[..., :3] > 0).any() and len(np.unique(ref_out.reshape(-1, ref_out.shape[-1]), axis=0)) > 16  # the knot shows
    assert (tri == tri_o).all() and bits_equal(t, t_o).all()


# -- c. Query.rebuild --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_leaf", SC.LEAVES)
@pytest.mark.parametrize("name", ["knot70k", "clusters"])
def test_query_rebuild_at_scale(torch, cases, name, max_leaf):
    """The rebuild, closest and occluded enqueued back to back on a non-default stream; then a second closest."""
    from srt_amd.query import Query

    scene, verts, built, order, rays, oracle = cases(name, max_leaf)
    n = len(scene.tris)
    assert n == SC.N_KNOT and SC.box_loop_threshold() < n <= SC.MERGE_LIMIT and n // 256 >= 272
    counts = RR.pair_height_counts(built)
    assert (counts > SC.LEVEL).sum() >= 3
    keys = BR.keys(scene, verts)
    if name == "clusters":
        assert len(np.unique(keys)) == 17 and (keys == keys[np.arange(n) % 17]).all()  # every key in every block
    else:
        assert len(np.unique(keys)) > n // 2
        assert SC.box_needs_the_tail(scene, verts, SC.box_loop_threshold())  # the loop's second pass decides the box
    depth_before, depth = LR.shape(scene.nodes)[2], LR.shape(built.nodes)[2]
    stream = torch.cuda.Stream()
    with Query(scene, stream=stream, refit=True, rebuild=True, rebuild_leaf=max_leaf) as q:
        in_hbm_before = q.get_int("stack.in_hbm")
        assert in_hbm_before == SC.in_hbm(depth_before) and q.get_int("scratch.bytes") == 256
        with torch.cuda.stream(stream):
            v = verts_dev(torch, verts)
            dev = to_dev(torch, rays)
            q.rebuild(v)
            hits = q.closest(dev)
            occ = q.occluded(dev)
        stream.synchronize()
        hits, occ = hits.numpy(), occ.cpu().numpy()
        assert q.get_int("stack.in_hbm") == SC.in_hbm(depth)
        if name == "knot70k":  # the rebuilt tree is deeper than 20: the stacks moved from LDS to HBM
            assert (in_hbm_before, q.get_int("stack.in_hbm")) == (0, 1)
            assert q.get_int("scratch.bytes") > 256
        with torch.cuda.stream(stream):
            again = q.closest(dev)  # the stack area allocated for the new plan, used again
        stream.synchronize()
        assert again.numpy().tobytes() == hits.tobytes()
        check_structure(q, built, order, walk=True)
        LT.check_counters(q, scene, built, max_leaf)
        assert q.get_int("refit.launches") >= 2 + 3 and q.get_int("rebuild.count") == 1
    hit = check_hits(built, order, hits, oracle)
    assert (occ == hit).all()
    assert hit.sum() >= 100, "the rays must find the mesh"


# -- d. no state carried over ------------------------------------------------------------------------------------------
def test_no_state_is_carried_between_rebuilds_at_scale(torch, cases):
    """A rebuild at other vertices and a query (its HBM stack area is live), a refit, then the rebuild at the test's
    vertices: the dwords and counters of a fresh object rebuilt once."""
    from srt_amd.query import Query

    scene, verts, built, order, rays, oracle = cases("knot70k", 4)
    assert len(scene.tris) > SC.box_loop_threshold()
    other = RR.wave(scene.verts, 1.5, 0.7)
    dev = to_dev(torch, rays)
    with Query(scene, refit=True, rebuild=True, rebuild_leaf=4) as q, Query(scene, refit=True, rebuild=True, rebuild_leaf=4) as once:
        q.rebuild(verts_dev(torch, other))
        first_order = q.tri_order()
        q.closest(dev)
        q.refit(verts_dev(torch, RR.wave(scene.verts, 0.4, 1.1)))
        q.rebuild(verts_dev(torch, verts))
        once.rebuild(verts)  # the numpy path uploads and synchronises
        for g, w in zip(q.layout(), once.layout()):
            assert g.shape == w.shape and (g == w).all()
        assert (q.tri_order() == once.tri_order()).all()
        assert not (first_order == order).all()  # (the first set of vertices gave another order)
        check_structure(q, built, order, walk=False)
        LT.check_counters(q, scene, built, 4)
        assert q.get_int("rebuild.count") == 2 and once.get_int("rebuild.count") == 1 and q.get_int("refit.count") == 1
        for key in STATE_KEYS:
            assert q.get_int(key) == once.get_int(key), key
        check_hits(built, order, q.closest(dev).numpy(), oracle)


# -- e. several records ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_leaf", SC.LEAVES)
def test_rebuild_of_two_records_at_scale(torch, cases, max_leaf):
    """The comparisons of tests/test_gpu_rebuild_models.py: the trees walked from every root and the ghost root, the pair
    numbering, the per-height counts of the schedule, and the hits with their record."""
    from srt_amd.query import Query

    scene, verts, built, order, rays, oracle = cases("knot70k_and_rubik", max_leaf)
    n = len(scene.tris)
    own = MR.owners(scene)
    assert len(scene.bvhs) == 2 and SC.box_loop_threshold() < n <= SC.MERGE_LIMIT
    assert (own[:SC.N_KNOT] == 0).all() and (own[SC.N_KNOT:] == 1).all() and SC.N_KNOT == 272 * 256  # 272 one-owner blocks
    assert (RR.pair_height_counts(built) > SC.LEVEL).sum() >= 3
    stream = torch.cuda.Stream()
    with Query(scene, stream=stream, refit=True, rebuild_models=True, rebuild_leaf=max_leaf) as q:
        with torch.cuda.stream(stream):
            v = verts_dev(torch, verts)
            dev = to_dev(torch, rays)
            q.rebuild(v)
            hits = q.closest(dev)
            occ = q.occluded(dev)
        stream.synchronize()
        hits, occ = hits.numpy(), occ.cpu().numpy()
        m = MT.check_structure(q, built, order, max_leaf)
        MT.check_counters(q, built, max_leaf, m)  # rebuild.height.<h> among them
        assert q.get_int("rebuild.count") == 1 and q.get_int("refit.launches") >= 2 + 3
        assert q.get_int("stack.in_hbm") == SC.in_hbm(q.get_int("rebuild.depth")) == 1
    hit = MT.check_hits(built, order, hits, oracle)
    assert (occ == hit).all() and hit.sum() >= 100


def test_rebuild_of_two_interleaved_records_at_scale(torch, cases):
    """Interleaved owners past one sort tile: "knot70k_and_rubik" with the runs of its leaves permuted in the triangle array,
    max_leaf 4, and the assertions of test_rebuild_of_two_records_at_scale.  Rubik's triangles lie in at least 100 of the
    277 blocks, so seg_box_kernel takes its mixed-owner path there, the 64-bit sort gathers a record from every tile, and
    pos_rec / seg / the hit remap work on owners that are nowhere contiguous in creation order."""
    from srt_amd.query import Query

    scene, verts, built, order, rays, oracle = cases("knot70k_and_rubik_shuffled", 4)
    n = len(scene.tris)
    own = MR.owners(scene)
    assert len(scene.bvhs) == 2 and SC.box_loop_threshold() < n <= SC.MERGE_LIMIT
    assert np.bincount(own).tolist() == [SC.N_KNOT, n - SC.N_KNOT]
    assert sum(1 for i in range(0, n, 256) if len(set(own[i:i + 256].tolist())) == 2) >= 100  # mixed-owner blocks
    assert (RR.pair_height_counts(built) > SC.LEVEL).sum() >= 3
    stream = torch.cuda.Stream()
    with Query(scene, stream=stream, refit=True, rebuild_models=True, rebuild_leaf=4) as q:
        with torch.cuda.stream(stream):
            v = verts_dev(torch, verts)
            dev = to_dev(torch, rays)
            q.rebuild(v)
            hits = q.closest(dev)
            occ = q.occluded(dev)
        stream.synchronize()
        hits, occ = hits.numpy(), occ.cpu().numpy()
        m = MT.check_structure(q, built, order, 4)
        MT.check_counters(q, built, 4, m)  # rebuild.height.<h> among them
        assert q.get_int("rebuild.records") == 2
        assert q.get_int("rebuild.count") == 1 and q.get_int("refit.launches") >= 2 + 3
        assert q.get_int("stack.in_hbm") == SC.in_hbm(q.get_int("rebuild.depth")) == 1
    hit = MT.check_hits(built, order, hits, oracle)
    assert (occ == hit).all() and hit.sum() >= 100


# -- f. onesweep -------------------------------------------------------------------------------------------------------
def test_rebuild_of_a_million_triangles(torch, cases):
    """Past 1,048,576 keys the radix sort is onesweep.  The vectorised checks alone, and the soup rebuilt where it was
    created, to keep the test near twice the time of tests/test_gpu_parity.py's 1 M-soup cases: measured in one run on an
    MI355X, 1.30 s beside 0.65 s (test_global_schedule_chosen_by_scene_size) and 0.58 s (test_launch_occupancy_reported);
    the 1,000 rays and their oracle cost 0.03 s of it."""
    from srt_amd.query import Query

    scene, verts, built, order, rays, oracle = cases("soup1m", 4)
    n = len(scene.tris)
    assert n == SC.N_SOUP > SC.MERGE_LIMIT and len(rays) == 1000
    root = built.nodes[0]["min"], built.nodes[0]["max"]  # box_partial_kernel's later passes decide the scene box
    assert SC.box_needs_the_tail(scene, verts, SC.box_loop_threshold(), box=root)
    m = (len(built.nodes) - 1) // 2
    counts = SC.height_counts(built.nodes)
    heights, launches = SC.schedule_of(counts)
    assert int(counts.sum()) == m and launches >= 2 + 3
    stream = torch.cuda.Stream()
    with Query(scene, stream=stream, refit=True, rebuild=True, rebuild_leaf=4) as q:
        with torch.cuda.stream(stream):
            v = verts_dev(torch, verts)
            dev = to_dev(torch, rays)
            q.rebuild(v)
            hits = q.closest(dev)
            occ = q.occluded(dev)
        stream.synchronize()
        hits, occ = hits.numpy(), occ.cpu().numpy()
        check_structure(q, built, order, walk=False)
        assert q.get_int("rebuild.pairs") == m and q.get_int("layout.pairs") == 64 * m
        assert q.get_int("rebuild.max_leaf") == int(built.nodes["count"].max()) <= 4
        assert q.get_int("rebuild.depth") == q.get_int("refit.heights") == heights
        assert q.get_int("refit.launches") == launches and q.get_int("rebuild.launches") == 10 + launches
        assert q.get_int("stack.entries") == heights + 1 and q.get_int("stack.in_hbm") == SC.in_hbm(heights)
        assert q.get_int("stack.packed") == 1 and q.get_int("rebuild.count") == 1
    hit = check_hits(built, order, hits, oracle)
    assert (occ == hit).all()
    assert hit.sum() >= 100, "the rays must find the mesh"
