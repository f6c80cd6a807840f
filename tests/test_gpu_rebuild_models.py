"""GPU: the device rebuild of a query object over several models (include/srt_rebuild_models.h,
Query(scene, refit=True, rebuild_models=True).rebuild) against the host mirror srt_bvh_build_lbvh_models -- the tree walked
from every root and from the ghost root, every box, .w dword and triangle record, the pair numbering, the schedule -- and
against the CPU oracle on the mirror's arrays, the hit position mapped through the order and the record checked.

tests/test_rebuild_models_api.py holds the mirror to the single-model mirror and to a numpy restatement of the rule; the
scenes are tests/rebuild_models_ref.py's: Rubik beside a small grid, three records (64 coincident triangles, one
triangle, three triangles), the first scene with its triangle blocks exchanged, and Rubik alone; for the structure also
three one-triangle models (no pair) and the grid unmoved, in the cube (the records' boxes overlap); and the many-record
scenes -- 4 to 300 small models, one of them large in "many_big", in creation order and with the records' triangles
interleaved -- for what depends on the number or the placement of the records: the sort's end bit, the roots loop of the
refit's tail past 256, seg_box_kernel's one-owner and mixed-owner blocks, owners that are not contiguous, ties between
coincident records, and the matrix of a high record.
"""
import dataclasses

import numpy as np
import pytest

import rebuild_leaf_ref as LR
import rebuild_models_ref as MR
import rebuild_ref as BR
import refit_ref as RR
import srt_amd as S
import surface_refit_ref as SRR
from conftest import OBJECTS, bits_equal
from oracle import pyoracle as O
from test_gpu_queries import MISS, to_dev
from test_gpu_rebuild import expected_schedule, verts_dev

pytestmark = pytest.mark.gpu

MULTI = ("two", "three", "swapped")
MANY_ALL = MR.MANY + MR.MANY_MIXED


def per_record(name):
    """check_hits' floor of rays per record: the many-record scenes have 64 rays a record, and check_many_found instead."""
    return 0 if name == "nested" or name.startswith("many") else 50


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


@pytest.fixture(scope="module")
def rubik():
    return S.load_obj(OBJECTS / "Rubik" / "Rubik.obj")


class Cases:
    """(scene, verts, mirror-built scene, order, rays, the oracle's answer on the mirror's arrays) per scene and max_leaf,
    made on first use and kept: the oracle traces each tree once."""

    def __init__(self, rubik):
        self.rubik, self.scenes, self.made = rubik, {}, {}

    def __call__(self, name, max_leaf):
        if name not in self.scenes:
            self.scenes[name] = MR.make_scene(name, self.rubik)
        if (name, max_leaf) not in self.made:
            scene, verts = self.scenes[name]
            built, order = S.build_lbvh_models(scene, verts, max_leaf=max_leaf)
            rays = MR.rays_of(name, scene, verts)
            self.made[name, max_leaf] = (scene, verts, built, order, rays, O.Oracle(built).trace_closest(len(built.bvhs), rays))
        return self.made[name, max_leaf]


@pytest.fixture(scope="module")
def cases(rubik):
    return Cases(rubik)


def check_hits(built, order, hits, oracle, per_record=50):
    """`hits`: HIT_DTYPE records of a rebuilt object; every field against the oracle on the mirror's arrays."""
    tri_o, t_o, n_o, st = oracle
    assert st["stack_overflow"] == 0
    hit = tri_o != MISS
    want = np.where(hit, order[np.where(hit, tri_o, 0)], MISS).astype(np.uint32)
    assert (hits["triangle"] == want).all(), f"{(hits['triangle'] != want).sum()} triangles differ"
    assert bits_equal(hits["t"], t_o).all()
    assert bits_equal(hits["normal"], n_o).all()
    assert (hits["material"][hit] == built.tris["mat"][tri_o[hit]]).all()
    record = MR.bvh_of_position(built)
    assert (hits["bvh"][hit] == record[tri_o[hit]]).all()
    assert (hits["bvh"][~hit] == 0).all() and (hits["material"][~hit] == 0).all()
    assert (hits["normal"][~hit].view(np.uint32) == 0).all()
    for r in range(len(built.bvhs)):
        assert (hits["bvh"][hit] == r).sum() >= per_record, f"the rays must find record {r}"
    return hit


def check_many_found(name, built, hits, hit):
    """A many-record scene: the object is in the regime the scene is named for, and the hits name every record but the
    later one of each coincident pair -- a record merged into its neighbour or lost would be missing here."""
    R = len(built.bvhs)
    assert R == (300 if "big" in name else int(name[4:].split("_")[0]))
    found = set(hits["bvh"][hit].tolist())
    assert sorted(set(range(R)) - found) == MR.many_exempt(R)
    assert (hits["material"][hit] == hits["bvh"][hit]).all()  # every model has a material of its own


def check_structure(q, built, order, max_leaf):
    """The device layout against the mirror: the walk from every root record and from the ghost root (leaf or not, first
    triangle, count, the six box dwords), the pair numbering of the rule, the triangle records and the order."""
    pairs, roots, tris = q.layout()
    n, records = len(built.tris), len(built.bvhs)
    assert roots.shape == (2 * (records + 1), 4)
    met_all, first = [], 0
    for r in range(records):
        got, met = MR.walk_layout(pairs, roots, r)
        BR.assert_same_tree(got, MR.walk_nodes(built.nodes, int(built.bvhs[r]["first_index"])))
        count = sum(g[3] for g in got)
        if max_leaf == 1:  # Karras' node k of record r is pair s_r + k; the root is pair s_r; index e_r is unused
            assert all(first <= p < first + count - 1 for p in met) and (not met or met[0] == first)
            if first + count - 1 < n - 1:
                assert (pairs[4 * (first + count - 1):4 * (first + count)] == 0).all()
        met_all += met
        first += count
    assert first == n
    assert (roots[2 * records:] == roots[0:2]).all()  # the ghost root is record 0's root
    m = len(met_all)
    assert len(set(met_all)) == m == (len(built.nodes) - records) // 2
    if max_leaf == 1:
        assert pairs.shape == (4 * (n - 1), 4)
    else:  # survivors ranked by increasing global index: dense, and every record's root before the next record's
        assert pairs.shape == (4 * max(m, 1), 4) and sorted(met_all) == list(range(m))
        if m == 0:
            assert (pairs == 0).all()
    assert (tris == BR.layout_tris(built)).all(), f"{(tris != BR.layout_tris(built)).sum()} tris dwords differ"
    assert (q.tri_order() == order).all()
    return m


def check_counters(q, built, max_leaf, m):
    records = len(built.bvhs)
    heights, launches = expected_schedule(built)
    depth = max(LR.shape(nodes)[2] for nodes in MR.blocks(built))
    assert heights == depth
    assert q.get_int("rebuild.models") == 1 and q.get_int("rebuild.records") == records and q.get_int("rebuild") == 1
    assert q.get_int("rebuild.leaf") == max_leaf and q.get_int("rebuild.pairs") == m
    assert q.get_int("rebuild.max_leaf") == int(built.nodes["count"].max()) and q.get_int("rebuild.depth") == depth
    assert q.get_int("stack.entries") == depth + 1 and q.get_int("stack.packed") == 1
    assert q.get_int("refit.heights") == heights and q.get_int("refit.launches") == launches
    # the schedule's pairs per height, as the device counted them, against the mirror's tree
    counts = RR.pair_height_counts(built) if len(built.nodes) > records else np.zeros(0, np.int64)
    assert [q.get_int(f"rebuild.height.{h}") for h in range(heights + 2)] == counts.tolist() + [0, 0]
    assert int(counts.sum()) == m
    # box, keys, sort, permute, then karras / range + scan + emit, climb, schedule
    assert q.get_int("rebuild.launches") == (7 if max_leaf == 1 else 9) + launches


@pytest.mark.parametrize("max_leaf", MR.LEAVES)
@pytest.mark.parametrize("name", MULTI + MR.EXTRA + MANY_ALL)
def test_structure_hits_and_counters_after_a_rebuild(torch, cases, name, max_leaf):
    """The rebuild, closest and occluded enqueued back to back on a non-default stream.  ("nested": no ray from outside
    meets the grid in the cube first, so that scene counts no hits per record.)

    The many-record scenes are here for: the sort's end bit, 32 + 2 | 3, 6 | 7 and 8 | 9 record bits at 4 | 5, 64 | 65 and
    256 | 257 records (one bit short merges two records' segments: the roots, the order and the hits' records differ); the
    roots loop of the refit's tail past its 256 lanes (257 and 300 records: n_roots of 258 and 301, every root and the
    ghost root compared); seg_box_kernel's blocks of one owner and the blocks straddling a record's ends ("many_big") and
    its blocks of a hundred owners and more (the shuffled scenes); and interleaved owners -- pos_rec, seg, segment_of,
    owner_of and the hit remap (the shuffled scenes: `triangle` is the creation index, `bvh` the record)."""
    from srt_amd.query import Query

    scene, verts, built, order, rays, oracle = cases(name, max_leaf)
    stream = torch.cuda.Stream()
    with Query(scene, stream=stream, refit=True, rebuild_models=True, rebuild_leaf=max_leaf) as q:
        assert q.get_int("rebuild.count") == 0 and q.get_int("rebuild.bytes") > 0
        assert (q.tri_order() == np.arange(len(scene.tris))).all()
        with torch.cuda.stream(stream):
            v = verts_dev(torch, verts)
            dev = to_dev(torch, rays)
            q.rebuild(v)
            hits = q.closest(dev)
            occ = q.occluded(dev)
        stream.synchronize()
        hits, occ = hits.numpy(), occ.cpu().numpy()
        m = check_structure(q, built, order, max_leaf)
        check_counters(q, built, max_leaf, m)
        assert q.get_int("rebuild.count") == 1
        if name.startswith("many"):
            assert q.get_int("rebuild.records") == len(scene.bvhs) and q.get_int("layout.roots") == 32 * (len(scene.bvhs) + 1)
    hit = check_hits(built, order, hits, oracle, per_record=per_record(name))
    assert (occ == hit).all()
    if name.startswith("many"):  # (few of the rays aimed at the whole lattice meet one of 4 or 5 small models)
        check_many_found(name, built, hits, hit)
    else:
        assert hit.sum() >= 100
    if name == "ones":  # no pair at all: check_structure saw the n - 1 unused slots (max_leaf 1) or the one pair zero
        assert m == 0


@pytest.mark.parametrize("name", MULTI + MR.MANY_HEAVY)
def test_rebuild_then_refit_keeps_the_topology(torch, cases, name):
    """(The many-record scenes: the refit over a device-built schedule of up to 300 trees, and its tail's roots loop past
    256 lanes at 257 and 300 records; the shuffled ones with the triangle records permuted against the creation order.)"""
    from srt_amd.query import Query

    scene, verts, built, order, rays, _ = cases(name, 4)
    other = RR.wave(verts, 0.4, 1.1)
    want = S.refit_scene(built, other)
    with Query(scene, refit=True, rebuild_models=True, rebuild_leaf=4) as q:
        q.rebuild(verts_dev(torch, verts))
        q.refit(verts_dev(torch, other))
        hits = q.closest(to_dev(torch, rays)).numpy()
        m = check_structure(q, want, order, 4)
        check_counters(q, want, 4, m)
        assert q.get_int("rebuild.count") == 1 and q.get_int("refit.count") == 1
    hit = check_hits(want, order, hits, O.Oracle(want).trace_closest(len(want.bvhs), rays), per_record=per_record(name))
    if name.startswith("many"):
        check_many_found(name, want, hits, hit)


BOTH_WAYS = ((4, 1), (1, 4))


@pytest.mark.parametrize("name,changes", [pytest.param(name, BOTH_WAYS, id=name) for name in MULTI + ("many257", "many_big_shuffled")] + [
    # m > 0 pairs (the record of 64), then every record a leaf root: m == 0 and pair 0 zeroed
    pytest.param("three", ((4, 255),), id="three-4-then-255")])
def test_no_state_is_carried_between_max_leaf_values(torch, cases, name, changes):
    """max_leaf 4 then 1 gives the dwords of a fresh max_leaf 1 object, and 1 then 4 those of a fresh max_leaf 4 one.
    ("many257": nine record bits in the sort and 258 roots; "many_big_shuffled": interleaved owners and mixed-owner blocks,
    the record boxes accumulated by atomics into words the second rebuild has to find zeroed again.)"""
    from srt_amd.query import Query

    keys = ("stack.entries", "stack.in_hbm", "stack.packed", "refit.heights", "refit.launches", "refit.bytes", "rebuild.depth",
            "rebuild.launches", "rebuild.pairs", "rebuild.max_leaf", "rebuild.leaf", "layout.pairs", "layout.roots",
            "layout.tris", "scene.bytes", "rebuild.records")
    for first, second in changes:
        scene, verts, built, order, rays, oracle = cases(name, second)
        with Query(scene, refit=True, rebuild_models=True, rebuild_leaf=first) as q, \
                Query(scene, refit=True, rebuild_models=True, rebuild_leaf=second) as once:
            q.rebuild(verts_dev(torch, RR.wave(scene.verts, 1.5, 0.7)))  # other vertices: another order
            q.set_rebuild_leaf(second)
            q.rebuild(verts_dev(torch, verts))
            once.rebuild(verts)  # the numpy path uploads and synchronises
            for g, w in zip(q.layout(), once.layout()):
                assert g.shape == w.shape and (g == w).all(), (first, second)
            assert (q.tri_order() == once.tri_order()).all()
            m = check_structure(q, built, order, second)
            check_counters(q, built, second, m)
            assert q.get_int("rebuild.count") == 2 and once.get_int("rebuild.count") == 1
            for key in keys:
                assert q.get_int(key) == once.get_int(key), (key, first, second)
            check_hits(built, order, q.closest(to_dev(torch, rays)).numpy(), oracle, per_record=per_record(name))


@pytest.mark.parametrize("max_leaf", MR.LEAVES)
def test_one_record_is_the_old_enable(torch, cases, max_leaf):
    """Scene (d): the new enable and the old one give identical layouts, counters and launches."""
    from srt_amd.query import Query

    scene, verts, built, order, rays, oracle = cases("single", max_leaf)
    keys = ("rebuild.launches", "rebuild.bytes", "rebuild.leaf_bytes", "rebuild.pairs", "rebuild.depth", "rebuild.max_leaf",
            "layout.pairs", "refit.launches", "refit.heights", "stack.entries", "scene.bytes")
    with Query(scene, refit=True, rebuild_models=True, rebuild_leaf=max_leaf) as q, \
            Query(scene, refit=True, rebuild=True, rebuild_leaf=max_leaf) as old:
        assert q.get_int("rebuild.models") == 1 and old.get_int("rebuild.models") == 0
        assert q.get_int("rebuild.records") == 1 and old.get_int("rebuild.records") == 1
        v = verts_dev(torch, verts)
        q.rebuild(v)
        old.rebuild(v)
        for g, w in zip(q.layout(), old.layout()):
            assert g.shape == w.shape and (g == w).all()
        assert (q.tri_order() == old.tri_order()).all() and (q.tri_order() == order).all()
        for key in keys:
            assert q.get_int(key) == old.get_int(key), key
        assert q.get_int("rebuild.launches") == (8 if max_leaf == 1 else 10) + expected_schedule(built)[1]
        dev = to_dev(torch, rays)
        assert (q.closest(dev).raw == old.closest(dev).raw).all()
    with Query(scene) as plain:
        assert plain.get_int("rebuild.models") == 0 and plain.get_int("rebuild.records") == 0


def test_a_moved_model_matrix_changes_the_hits_as_on_a_created_object(torch, cases):
    from srt_amd.query import Query

    scene, verts, built, order, rays, _ = cases("two", 4)
    frame = np.eye(4, dtype=np.float32)
    frame[3, :3] = (-3.0, 1.5, 2.0)  # world -> model frame of the grid (glm column 3)
    moved = dataclasses.replace(built, bvhs=built.bvhs.copy())
    moved.bvhs[1]["frame"] = frame.reshape(16)
    dev = to_dev(torch, rays)
    with Query(scene, refit=True, rebuild_models=True, rebuild_leaf=4) as q, Query(moved) as created:
        q.rebuild(verts_dev(torch, verts))
        before = q.closest(dev).numpy()
        q.update_model_matrix(1, frame)
        hits = q.closest(dev).numpy()
        # (the rays were aimed at the grid where it was: fewer find it now)
        check_hits(moved, order, hits, O.Oracle(moved).trace_closest(2, rays), per_record=10)
        assert (hits["t"].view(np.uint32) != before["t"].view(np.uint32)).sum() >= 50
        want = created.closest(dev).numpy()  # an object created from the mirror's arrays: positions, not creation indices
        hit = want["triangle"] != MISS
        assert (hits["triangle"][hit] == order[want["triangle"][hit]]).all() and (hits["triangle"][~hit] == MISS).all()
        for field in ("t", "normal", "material", "bvh"):
            assert hits[field].tobytes() == want[field].tobytes(), field


@pytest.mark.parametrize("name", ("many300", "many_big_shuffled"))
@pytest.mark.parametrize("max_leaf", MR.LEAVES)
def test_a_tie_between_coincident_records_goes_to_the_first_visited(torch, cases, name, max_leaf):
    """Ties across records: records 40, 45, 50 and 55 repeat records 3, 4, 5 and 7 triangle for triangle where they stand,
    so every ray that meets one meets the other at the same t.  The closest hit keeps the first visited -- the roots are
    visited in record order -- after a rebuild as inside one tree: `bvh` is the record the oracle reports on the mirror's
    arrays, the earlier one, for at least one ray of every pair."""
    from srt_amd.query import Query

    scene, verts, built, order, rays, oracle = cases(name, max_leaf)
    pairs = MR.many_pairs(len(scene.bvhs))
    assert len(pairs) >= 4
    tri_o = oracle[0]
    hit = tri_o != MISS
    record = np.where(hit, MR.bvh_of_position(built)[np.where(hit, tri_o, 0)], MISS)
    with Query(scene, refit=True, rebuild_models=True, rebuild_leaf=max_leaf) as q:
        q.rebuild(verts_dev(torch, verts))
        assert q.get_int("rebuild.records") == len(scene.bvhs)
        hits = q.closest(to_dev(torch, rays)).numpy()
    own = MR.owners(scene)
    for later, earlier in pairs.items():
        tied = (record == earlier) | (record == later)
        assert tied.sum() >= 1, f"no ray finds the pair ({earlier}, {later})"
        assert (record[tied] == earlier).all()  # the oracle alone: the first visited
        assert (hits["bvh"][tied] == earlier).all() and (hits["material"][tied] == earlier).all()
        assert (own[hits["triangle"][tied]] == earlier).all()  # the creation index is one of the earlier record's
        assert bits_equal(hits["t"][tied], oracle[1][tied]).all()


def small_frame(r):
    """A world -> model translation of its own for record r, a twentieth of a triangle's size: rays aimed at the record
    still find it (record 255 is one triangle), at another t."""
    frame = np.eye(4, dtype=np.float32)
    frame[3, :3] = (0.05 + 0.0001 * r, -0.04, 0.03 + 0.001 * (r % 7))
    return frame


def test_matrices_of_high_records_after_a_rebuild(torch, cases):
    """A high record's matrix: after a rebuild of 300 records, update_model_matrix on records 0, 255, 256 and 299 -- the
    first, the last of the first 256 roots, the first past them and the last -- gives the hits of an object created from
    the mirror's scene with the same matrices, and the oracle's."""
    from srt_amd.query import Query

    scene, verts, built, order, rays, oracle = cases("many300", 4)
    moved_records = (0, 255, 256, 299)
    moved = dataclasses.replace(built, bvhs=built.bvhs.copy())
    for r in moved_records:
        moved.bvhs[r]["frame"] = small_frame(r).reshape(16)
    dev = to_dev(torch, rays)
    tri_m = O.Oracle(moved).trace_closest(300, rays)[0]  # the oracle alone: the rays find the four where they moved to
    found = MR.bvh_of_position(moved)[tri_m[tri_m != MISS]]
    assert all((found == r).sum() >= 1 for r in moved_records)
    with Query(scene, refit=True, rebuild_models=True, rebuild_leaf=4) as q, Query(moved) as created:
        q.rebuild(verts_dev(torch, verts))
        assert q.get_int("rebuild.records") == 300 > max(moved_records) >= 256
        before = q.closest(dev).numpy()
        for r in moved_records:
            q.update_model_matrix(r, small_frame(r))
        hits = q.closest(dev).numpy()
        want = created.closest(dev).numpy()  # positions of the mirror's arrays, not creation indices
    hit = check_hits(moved, order, hits, O.Oracle(moved).trace_closest(300, rays), per_record=0)
    for r in moved_records:
        mine = hit & (hits["bvh"] == r)
        assert mine.sum() >= 1, f"no ray finds record {r} where it moved to"
        assert (hits["t"][mine].view(np.uint32) != before["t"][mine].view(np.uint32)).any()
    others = hit & ~np.isin(hits["bvh"], moved_records) & (before["bvh"] == hits["bvh"]) & (before["triangle"] == hits["triangle"])
    assert others.sum() >= 1000 and (hits["t"][others].view(np.uint32) == before["t"][others].view(np.uint32)).all()
    assert (hits["triangle"][hit] == order[want["triangle"][hit]]).all() and (want["triangle"][~hit] == MISS).all()
    for field in ("t", "normal", "material", "bvh"):
        assert hits[field].tobytes() == want[field].tobytes(), field


def test_a_surface_object_shades_the_hits_of_300_rebuilt_records(torch, cases):
    """The downstream stage on many records.  A Surface object created before the rebuild, refit to
    the same vertices, shades the rebuilt object's hits as tests/surface_ref.py says on those vertices.  Every model has
    a diffuse colour of its own, so a `bvh` or a `triangle` that is off by one record changes the albedo: the albedo of
    every hit is its record's colour."""
    from srt_amd.query import Query
    from srt_amd.surface import ATTR_DTYPE, Surface

    scene, verts, built, order, rays, oracle = cases("many300", 4)
    dev = to_dev(torch, rays)
    with Surface(scene, refit=True) as surf, Query(scene, refit=True, rebuild_models=True, rebuild_leaf=4) as q:
        vd = verts_dev(torch, verts)
        q.rebuild(vd)
        surf.refit(vd)
        assert q.get_int("rebuild.records") == 300
        h = q.closest(dev)
        out = surf.shade(dev, h)
        surf.synchronize()
        got, hits = out.cpu().numpy().view(ATTR_DTYPE).reshape(-1), h.numpy()
    hit = check_hits(built, order, hits, oracle, per_record=0)
    want = SRR.shade_refit(scene, verts, rays, hits, tex_albedo=scene.tex_albedo)
    assert (got.view(np.uint32) == want.view(np.uint32)).all()
    assert (got["hit"] == hit).all() and hit.sum() >= 1000
    colour = np.asarray([MR.many_kd(r) for r in range(300)], np.float32)
    assert (got["albedo"][hit] == colour[hits["bvh"][hit]]).all()
    assert len(np.unique(got["albedo"][hit], axis=0)) == 300 - len(MR.many_exempt(300))


def test_refusals_enqueue_nothing_and_leave_the_layout(torch, cases):
    from srt_amd import SrtError, _lib
    from srt_amd.query import Query

    scene, verts, built, order, rays, oracle = cases("two", 1)

    def invalid(call, text):
        with pytest.raises(SrtError) as e:
            call()
        assert e.value.code == _lib.SRT_ERR_INVALID and text in str(e.value), str(e.value)

    shared = dataclasses.replace(scene, bvhs=scene.bvhs.copy())
    shared.bvhs[1]["first_index"] = 0
    orphan = dataclasses.replace(scene, tris=np.concatenate([scene.tris, scene.tris[:1]]))
    late = dataclasses.replace(scene, bvhs=scene.bvhs[::-1].copy())
    for bad, text in ((shared, "every triangle must belong to exactly one BVH record"),
                      (orphan, "every triangle must belong to exactly one BVH record"), (late, "first_index is not 0")):
        with Query(bad, refit=True) as q:
            before = q.layout()
            invalid(q.enable_rebuild_models, text)
            assert q.get_int("rebuild") == 0 and q.get_int("rebuild.models") == 0 and q.get_int("rebuild.bytes") == 0
            invalid(lambda: q.rebuild(verts_dev(torch, bad.verts)), "not enabled")
            for g, w in zip(q.layout(), before):
                assert g.shape == w.shape and (g == w).all()
        with pytest.raises(SrtError):
            Query(bad, refit=True, rebuild_models=True)
    with Query(scene) as plain:
        invalid(plain.enable_rebuild_models, "SRT_QUERY_REFIT")
    # the old entry point keeps refusing two records, and the new one takes the object afterwards
    with pytest.raises(SrtError, match="more than one BVH record"):
        Query(scene, refit=True, rebuild=True)
    with Query(scene, refit=True) as q:
        before = q.layout()
        invalid(q.enable_rebuild, "more than one BVH record")
        for g, w in zip(q.layout(), before):
            assert (g == w).all()
        q.enable_rebuild_models()
        q.enable_rebuild_models()  # a second call changes nothing
        bytes_before = q.get_int("rebuild.bytes")
        invalid(lambda: q.rebuild(verts_dev(torch, verts)[:-1].contiguous()), "n_verts")
        assert q.get_int("rebuild.count") == 0 and q.get_int("rebuild.bytes") == bytes_before
        for g, w in zip(q.layout(), before):
            assert (g == w).all()
        q.rebuild(verts_dev(torch, verts))
        check_structure(q, built, order, 1)


def test_surface_and_temporal_objects_stay_valid(torch, cases):
    """srt_hit.triangle stays the scene's triangle index and srt_hit.bvh the record after a rebuild of two models: a Surface
    and a Temporal object built from the scene give, on the rebuilt query's hits, bit for bit what they give on the hits of
    a query that was only refit to the same vertices.  Rays that hit two triangles at one distance are dropped on the CPU."""
    from srt_amd.query import Query
    from srt_amd.surface import Surface
    from srt_amd.temporal import Temporal

    scene, verts, _, _, _, _ = cases("two", 4)
    W, H = 64, 40
    frames = [verts, RR.wave(scene.verts, 0.3, 0.9)]
    rays = MR.scene_rays(scene, verts, per_record=900, seed=404)
    rays = rays[np.random.default_rng(7).permutation(len(rays))]  # (the cut below keeps rays of every kind)
    keep = np.ones(len(rays), bool)
    for v in frames:  # the oracle alone: where the two trees name different triangles, two lie at one distance
        b, o = S.build_lbvh_models(scene, v, max_leaf=4)
        tri_b, t_b, _, _ = O.Oracle(b).trace_closest(2, rays)
        tri_r, t_r, _, _ = O.Oracle(S.refit_scene(scene, v)).trace_closest(2, rays)
        assert bits_equal(t_b, t_r).all()
        keep &= np.where(tri_b != MISS, o[np.where(tri_b != MISS, tri_b, 0)], MISS) == tri_r
    assert (~keep).mean() <= 0.01
    rays = rays[keep][:W * H]
    assert len(rays) == W * H
    cam = ((0.0, 0.0, 30.0), (0.0, 0.0, -1.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0))
    rng = np.random.default_rng(5)
    dev = to_dev(torch, rays)
    with Query(scene, refit=True, rebuild_models=True, rebuild_leaf=4) as qb, Query(scene, refit=True) as qr, \
            Surface(scene, refit=True) as surf, Temporal(W, H) as tb, Temporal(W, H) as tr:
        tb.set_mesh(scene)
        tr.set_mesh(scene)
        for k, v in enumerate(frames):
            vd = verts_dev(torch, v)
            qb.rebuild(vd)
            qr.refit(vd)
            surf.refit(vd)
            hb, hr = qb.closest(dev), qr.closest(dev)
            assert (hb.raw == hr.raw).all() and 0.25 < float(hb.hit.float().mean()) < 0.95
            assert int((hb.bvh[hb.hit] == 1).sum()) >= 50 and int((hb.bvh[hb.hit] == 0).sum()) >= 50
            assert (surf.shade(dev, hb) == surf.shade(dev, hr)).all()
            acc = np.ones((H, W, 4), np.float32)
            acc[..., :3] = rng.uniform(0, 6, (H, W, 3)).astype(np.float32)
            acc = torch.from_numpy(acc).cuda()
            tb.set_vertices(vd)
            tr.set_vertices(vd)
            a, b = tb.accumulate(acc, 3, hb, cam), tr.accumulate(acc, 3, hr, cam)
            assert (a.view(torch.int32) == b.view(torch.int32)).all(), f"frame {k}"
