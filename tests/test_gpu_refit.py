"""GPU: the device refit of a query object (include/srt_refit.h, Query(scene, refit=True).refit) against the fresh
layout, in every dword, and against the CPU oracle.

`Qd` is Query(scene, refit=True) after refit(verts'); `Qf` a fresh Query(refit_scene(scene, verts')), whose nodes the
host refit srt_bvh_refit made (tests/test_refit_api.py holds that one to a numpy restatement).  layout() returns the
device arrays pairs / roots / tris as uint32 [n, 4]; the roots include the ghost record (node 0).
"""
import numpy as np
import pytest

import rebuild_models_ref as MR
import refit_ref as RR
import srt_amd as S
from conftest import OBJECTS
from oracle import pyoracle as O
from test_gpu_queries import MISS, bounds, check_closest, rubik_rays, sphere_rays, to_dev

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


@pytest.fixture(scope="module")
def rubik():
    return S.load_obj(OBJECTS / "Rubik" / "Rubik.obj")


@pytest.fixture(scope="module")
def rubik_scene(rubik):
    return S.Scene.from_models([rubik])


@pytest.fixture(scope="module")
def rubik_case(rubik_scene):
    """Rubik, its deformed vertices, the host-refit scene, 4099 rays and the oracle's answers on both meshes."""
    verts = RR.wave(rubik_scene.verts)
    refit = S.refit_scene(rubik_scene, verts)
    rays = rubik_rays(rubik_scene, 4099)
    tri0, t0, _, _ = O.Oracle(rubik_scene).trace_closest(1, rays)
    tri1, t1, _, _ = O.Oracle(refit).trace_closest(1, rays)
    return verts, refit, rays, (tri0, t0), (tri1, t1)


def verts_dev(torch, verts):
    return torch.from_numpy(verts.view(np.float32).reshape(-1, 8).copy()).cuda()


def same_centroid_triangles():
    """5 triangles of different shapes whose corners each sum to exactly zero: one centroid, so one leaf of 5."""
    tri = []
    for k in range(5):
        a, b = np.array([k + 1.0, 0.5 * k, -1.0]), np.array([-2.0, k + 2.0, 0.25 * k])
        tri.append([a, b, -(a + b)])
    return np.asarray(tri, np.float32).reshape(-1, 9)


def small_scene(name, rubik):
    if name == "rubik":
        return S.Scene.from_models([rubik])
    if name == "grid":
        return S.Scene.from_models([S.model_from_triangles(RR.grid_triangles())])
    if name == "one":
        return S.Scene.from_models([S.model_from_triangles(RR.grid_triangles(1)[:1])])
    if name == "two":
        return S.Scene.from_models([S.model_from_triangles(RR.grid_triangles(1))])
    if name == "five":
        return S.Scene.from_models([S.model_from_triangles(same_centroid_triangles())])
    if name.startswith("many"):  # tests/rebuild_models_ref.py's many-record scenes, as the loader's builder made them
        return MR.make_scene(name, rubik)[0]
    assert name == "two_models"
    return S.Scene.from_models([rubik, S.model_from_triangles(RR.grid_triangles(5))])


def assert_layouts_equal(got, want):
    for g, w, what in zip(got, want, ("pairs", "roots", "tris")):
        assert g.shape == w.shape and g.dtype == w.dtype == np.uint32, what
        assert (g == w).all(), f"{what}: {(g != w).sum()} dwords differ"


@pytest.mark.parametrize("name", ["rubik", "grid", "one", "two", "five", "two_models", "many257", "many_big_shuffled"])
def test_every_dword_equals_the_fresh_layout(torch, rubik, name):
    """("many257", "many_big_shuffled": the roots loop of the tail's block past its 256 lanes -- 258 and 301 root records,
    the ghost root the last -- and in the second the triangle records of interleaved owners.)"""
    from srt_amd.query import Query

    scene = small_scene(name, rubik)
    verts = RR.wave(scene.verts, 0.25, 0.3)
    with Query(scene, refit=True) as qd, Query(S.refit_scene(scene, verts)) as qf:
        before = qd.layout()
        assert qd.get_int("refit") == 1 and qd.get_int("refit.count") == 0
        heights, launches = qd.get_int("refit.heights"), qd.get_int("refit.launches")
        n_pairs = (len(scene.nodes) - len(scene.bvhs)) // 2  # (a tree of 2 m + 1 nodes a record)
        assert qd.get_int("refit.bytes") >= 16 * len(scene.tris) + 4 * n_pairs
        # the schedule, from the nodes alone: a launch for the triangles, one for each level under the maximal
        # suffix of levels of at most 256 pairs, and the one-block tail
        counts = RR.pair_height_counts(scene)
        tail_begin = len(counts)
        while tail_begin > 0 and counts[tail_begin - 1] <= 256:
            tail_begin -= 1
        assert heights == len(counts) and launches == 2 + tail_begin
        if name == "grid":
            # more than 256 pairs at height 0: at least one launch of a level precedes the one-block tail
            assert len(scene.tris) == 1152 and counts[0] > 256
            assert launches >= 3 and heights > launches - 2
        elif name == "one":
            assert len(scene.nodes) == 1 and heights == 0 and launches == 2  # the root is a leaf: no pairs
        elif name == "two":
            assert len(scene.tris) == 2
        elif name == "five":
            assert scene.nodes["count"].max() == 5 and len(scene.nodes) == 1
        elif name == "two_models":
            frame = np.eye(4, dtype=np.float32)
            frame[3, :3] = (3.0, -2.0, 1.0)
            qd.update_model_matrix(1, frame)
            assert before[1].shape == (2 * 3, 4)  # two records and the ghost root
        elif name.startswith("many"):
            n_roots = qd.get_int("layout.roots") // 32  # two float4 a root record
            assert n_roots == len(scene.bvhs) + 1 > 256 and before[1].shape == (2 * n_roots, 4)
            assert (before[1][2 * 256:, :3] != 0).any()  # (boxes past the first 256 roots, which the refit must move)
        qd.refit(verts_dev(torch, verts))
        assert qd.get_int("refit.count") == 1
        got, want = qd.layout(), qf.layout()
        assert_layouts_equal(got, want)
        assert not (got[1] == before[1]).all() and not (got[2] == before[2]).all()  # and it is no no-op
        assert (got[2][-3:] == 0).all()  # the pad record
        if name.startswith("many"):  # every root past the tail block's first trip moved too
            moved = (got[1][0::2, :3] != before[1][0::2, :3]).any(1) | (got[1][1::2, :3] != before[1][1::2, :3]).any(1)
            assert moved[256:].all() and moved.all()


def test_hits_after_a_refit_match_the_oracle(torch, rubik_scene, rubik_case):
    """refit and the queries enqueued back to back on a non-default stream, nothing between them."""
    from srt_amd.query import Query

    verts, refit, rays, (tri0, t0), (tri1, t1) = rubik_case
    # the oracle alone, before any GPU call: the deformation is one a no-op refit cannot pass for
    both = (tri0 != MISS) & (tri1 != MISS)
    assert both.sum() > 1000
    assert (t0[both].view(np.uint32) != t1[both].view(np.uint32)).mean() >= 0.5
    assert ((tri0 != tri1) | ((tri0 == MISS) != (tri1 == MISS))).mean() >= 0.05
    stream = torch.cuda.Stream()
    with Query(rubik_scene, stream=stream, refit=True) as q:
        q.set_bvh_count(1)
        with torch.cuda.stream(stream):
            v = verts_dev(torch, verts)
            dev = to_dev(torch, rays)
            q.refit(v)
            hits = q.closest(dev)
            occ = q.occluded(dev)
        stream.synchronize()
        hits, occ = hits.numpy(), occ.cpu().numpy()
    tri_o, _ = check_closest(refit, 1, rays, hits)
    assert (tri_o == tri1).all()
    assert (occ == (tri_o != MISS)).all()


def test_hits_after_a_refit_of_300_records(torch, rubik):
    """The roots loop past 256: a refit of "many300" -- 301 root records, so the tail's block takes a second trip over its
    256 lanes -- then closest and occluded; every field against the oracle on the host-refit scene, the records 256 to
    299 among the hits."""
    from srt_amd.query import Query

    scene, verts = MR.make_scene("many300", rubik)
    rays = MR.rays_of("many300", scene, verts)
    own = MR.owners(scene)
    with Query(scene, refit=True) as q:
        n_roots = q.get_int("layout.roots") // 32
        assert n_roots == 301 > 256
        dev = to_dev(torch, rays)
        q.refit(verts_dev(torch, verts))
        hits = q.closest(dev).numpy()
        occ = q.occluded(dev).cpu().numpy()
    tri_o, _ = check_closest(S.refit_scene(scene, verts), 300, rays, hits, bvh_of=lambda tri: own[tri].astype(np.uint32))
    hit = tri_o != MISS
    assert (occ == hit).all()
    found = set(hits["bvh"][hit].tolist())
    assert sorted(set(range(300)) - found) == MR.many_exempt(300) and set(range(256, 300)) <= found


def test_two_models_hits_after_a_refit(torch, rubik):
    """The moved record's matrix survives the refit, and the hits of both records follow the new vertices."""
    from srt_amd.query import Query

    scene = small_scene("two_models", rubik)
    n0 = len(S.Scene.from_models([rubik]).tris)
    verts = RR.wave(scene.verts)
    frame = np.eye(4, dtype=np.float32)
    frame[3, :3] = (12.0, -2.0, -5.0)
    lo, hi = bounds(S.Scene.from_models([rubik]))
    glo, ghi = np.array((0.0, 0.0, -0.5)) - (12.0, -2.0, -5.0), np.array((5.0, 5.0, 0.5)) - (12.0, -2.0, -5.0)
    rays = np.concatenate([sphere_rays(lo, hi, 1000, 41), sphere_rays(glo, ghi, 1000, 42, spread=1.2)])
    with Query(scene, refit=True) as q:
        q.update_model_matrix(1, frame)
        q.refit(verts_dev(torch, verts))
        hits = q.closest(to_dev(torch, rays)).numpy()
    refit = S.refit_scene(scene, verts)
    refit.bvhs[1]["frame"] = frame.reshape(16)
    tri_o, _ = check_closest(refit, 2, rays, hits, bvh_of=lambda tri: (tri >= n0).astype(np.uint32))
    assert ((tri_o != MISS) & (tri_o < n0)).sum() > 200 and ((tri_o != MISS) & (tri_o >= n0)).sum() > 200


def test_no_state_is_carried_between_refits(torch, rubik_scene):
    from srt_amd.query import Query

    a, b = RR.wave(rubik_scene.verts, 0.4, 1.1), RR.wave(rubik_scene.verts)
    with Query(rubik_scene, refit=True) as q, Query(rubik_scene, refit=True) as only_b, Query(rubik_scene) as fresh:
        q.refit(verts_dev(torch, a))
        after_a = q.layout()
        q.refit(verts_dev(torch, b))
        only_b.refit(b)  # the numpy path uploads and synchronises
        assert_layouts_equal(q.layout(), only_b.layout())
        assert not (after_a[0] == q.layout()[0]).all()
        assert q.get_int("refit.count") == 2 and only_b.get_int("refit.count") == 1
        # back to the builder's vertices: the builder's boxes as values (a zero's sign may differ), the rest in bits
        q.refit(verts_dev(torch, rubik_scene.verts))
        got, want = q.layout(), fresh.layout()
        for g, w in zip(got[:2], want[:2]):
            assert (g.view(np.float32)[:, :3] == w.view(np.float32)[:, :3]).all()
            assert (g[:, 3] == w[:, 3]).all()
        assert (got[2] == want[2]).all()


def test_an_object_without_the_flag_is_as_before(torch, rubik_scene, rubik_case):
    from srt_amd import SrtError, _lib
    from srt_amd.query import Query

    rays = rubik_case[2][:129]
    with Query(rubik_scene) as plain, Query(rubik_scene, refit=True) as flagged:
        for name in ("refit", "refit.bytes", "refit.heights", "refit.launches", "refit.count"):
            assert plain.get_int(name) == 0
        assert flagged.get_int("refit") == 1 and flagged.get_int("refit.bytes") > 16 * len(rubik_scene.tris)
        assert_layouts_equal(plain.layout(), flagged.layout())
        sizes = [plain.get_int("layout." + n) for n in ("pairs", "roots", "tris")]
        assert sizes == [64 * ((len(rubik_scene.nodes) - 1) // 2), 32 * 2, 48 * (len(rubik_scene.tris) + 1)]
        for q in (plain, flagged):
            q.set_bvh_count(1)
            q.closest(to_dev(torch, rays))
            # what the object held and launched before the refit existed (Rubik: LDS stacks, no HBM scratch)
            assert q.get_int("scratch.bytes") == 256 and q.get_int("stack.in_hbm") == 0
            assert q.get_int("launch.blocks") == 1 and q.get_int("launch.block") == 256
            assert q.get_int("scene.bytes") == sum(sizes) + 2 * 64
        with pytest.raises(SrtError) as e:
            plain.refit(verts_dev(torch, rubik_scene.verts))
        assert e.value.code == _lib.SRT_ERR_INVALID and "without SRT_QUERY_REFIT" in str(e.value)
        del e  # (its traceback holds this frame: no cycle is left to keep the tensors past the test)
        assert plain.get_int("refit.count") == 0
        assert_layouts_equal(plain.layout(), flagged.layout())


def test_argument_errors_enqueue_nothing(torch, rubik_scene):
    from srt_amd import SrtError, _lib
    from srt_amd.query import Query

    n = len(rubik_scene.verts)
    good = verts_dev(torch, RR.wave(rubik_scene.verts))
    with Query(rubik_scene, refit=True) as q:
        before = q.layout()
        for bad in (torch.cat([good, good[:1]]), good[:-1].contiguous()):  # a wrong n_verts
            with pytest.raises(SrtError) as e:
                q.refit(bad)
            assert e.value.code == _lib.SRT_ERR_INVALID and q.get_int("refit.count") == 0
        del e, bad  # (the traceback holds this frame: no cycle is left to keep the tensors past the test)
        flat = torch.zeros(8 * n + 1, dtype=torch.float32, device="cuda")
        view = flat[1:].view(n, 8)  # contiguous, 4 B past a 16-B boundary
        assert view.is_contiguous() and view.data_ptr() % 16 == 4
        with pytest.raises(SrtError) as e:
            q.refit(view)
        assert e.value.code == _lib.SRT_ERR_INVALID and q.get_int("refit.count") == 0
        del e
        with pytest.raises(ValueError):
            q.refit(good.cpu())
        with pytest.raises(ValueError):
            q.refit(good.to(torch.float64))
        assert q.get_int("refit.count") == 0
        assert_layouts_equal(q.layout(), before)
        q.refit(good)
        assert q.get_int("refit.count") == 1
