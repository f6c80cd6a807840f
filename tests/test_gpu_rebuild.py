"""GPU: the device rebuild of a query object (include/srt_rebuild.h, Query(scene, refit=True, rebuild=True).rebuild)
against the host mirror srt_bvh_build_lbvh -- the tree walked from the root, every box and triangle dword -- and
against the CPU oracle on the host-built arrays, the oracle's hit position mapped through the order.

tests/test_rebuild_api.py holds the host mirror to a numpy restatement of the rule; tests/rebuild_ref.py has the scenes:
Rubik; a 24 x 24 quad grid, flat (no extent in z) and lifted (more than 256 height-0 pairs: a per-level refit launch and
the fused tail both run); 64 copies of one triangle (every key equal); 1, 2 and 3 triangles; a mesh with two vertex
indices out of range.
"""
import dataclasses

import numpy as np
import pytest

import rebuild_ref as BR
import refit_ref as RR
import special_rays as SR
import srt_amd as S
from conftest import OBJECTS, bits_equal
from oracle import pyoracle as O
from test_gpu_queries import MISS, bounds, sphere_rays, to_dev

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


@pytest.fixture(scope="module")
def rubik():
    return S.load_obj(OBJECTS / "Rubik" / "Rubik.obj")


def verts_dev(torch, verts):
    return torch.from_numpy(verts.view(np.float32).reshape(-1, 8).copy()).cuda()


def scene_rays(name, built):
    """Rays for one scene: generic ones from outside the box and ones aimed at triangles; on Rubik also every family
    of tests/special_rays.py (on-plane, axis-parallel, epsilon distances, NaN / Inf), made for the built tree's boxes."""
    lo, hi = bounds(built)
    hi = np.maximum(hi, lo + 1e-3)
    if name == "oob":  # (triangle_rays indexes the vertices itself: not with an index out of range)
        return np.concatenate([sphere_rays(lo, hi, 1500, 11), sphere_rays(lo, hi, 600, 12, spread=0.8)])
    sets = [sphere_rays(lo, hi, 1500, 11), SR.triangle_rays(built, 600, 12)]
    if name == "rubik":
        sets.append(SR.concat(list(SR.all_families(built).values()))[0])
    return np.concatenate(sets)


@pytest.fixture(scope="module")
def cases(rubik):
    """{name: (scene, verts, host-built scene, order, rays, the oracle's answer on the host-built scene)}, once."""
    out = {}
    for name in BR.SCENES:
        scene, verts = BR.make_scene(name, rubik)
        built, order = S.build_lbvh(scene, verts)
        rays = scene_rays(name, built)
        out[name] = (scene, verts, built, order, rays, O.Oracle(built).trace_closest(1, rays))
    return out


def check_hits(built, order, hits, oracle):
    """`hits`: HIT_DTYPE records of a rebuilt object; every field against the oracle on the host-built scene."""
    tri_o, t_o, n_o, st = oracle
    assert st["stack_overflow"] == 0
    hit = tri_o != MISS
    want = np.where(hit, order[np.where(hit, tri_o, 0)], MISS).astype(np.uint32)
    assert (hits["triangle"] == want).all(), f"{(hits['triangle'] != want).sum()} triangles differ"
    assert bits_equal(hits["t"], t_o).all()
    assert bits_equal(hits["normal"], n_o).all()
    assert (hits["material"][hit] == built.tris["mat"][tri_o[hit]]).all()
    assert (hits["bvh"] == 0).all()
    assert (hits["material"][~hit] == 0).all() and (hits["normal"][~hit].view(np.uint32) == 0).all()
    return hit


def check_structure(q, built, order):
    pairs, roots, tris = q.layout()
    BR.assert_same_tree(BR.walk_layout(pairs, roots), BR.walk_nodes(built.nodes))
    assert (roots[2:4] == roots[0:2]).all()  # the ghost root is the root
    assert pairs.shape == (4 * max(len(built.tris) - 1, 1), 4)
    assert (tris == BR.layout_tris(built)).all(), f"{(tris != BR.layout_tris(built)).sum()} tris dwords differ"
    assert (q.tri_order() == order).all()


def expected_schedule(built):
    """(heights, launches of one refit) of the built tree, from its nodes alone."""
    counts = RR.pair_height_counts(built) if len(built.nodes) > 1 else np.zeros(0, np.int64)
    tail_begin = len(counts)
    while tail_begin > 0 and counts[tail_begin - 1] <= 256:
        tail_begin -= 1
    return len(counts), 2 + tail_begin


@pytest.mark.parametrize("name", BR.SCENES)
def test_structure_and_hits_after_a_rebuild(torch, cases, name):
    """The rebuild, closest and occluded enqueued back to back on a non-default stream: nothing between them but the
    rebuild's own synchronisation."""
    from srt_amd.query import Query

    scene, verts, built, order, rays, oracle = cases[name]
    stream = torch.cuda.Stream()
    with Query(scene, stream=stream, refit=True, rebuild=True) as q:
        assert q.get_int("rebuild") == 1 and q.get_int("rebuild.count") == 0 and q.get_int("rebuild.bytes") > 0
        assert (q.tri_order() == np.arange(len(scene.tris))).all()
        with torch.cuda.stream(stream):
            v = verts_dev(torch, verts)
            dev = to_dev(torch, rays)
            q.rebuild(v)
            hits = q.closest(dev)
            occ = q.occluded(dev)
        stream.synchronize()
        hits, occ = hits.numpy(), occ.cpu().numpy()
        check_structure(q, built, order)
        heights, launches = expected_schedule(built)
        assert q.get_int("rebuild.count") == 1 and q.get_int("rebuild.depth") == heights
        assert q.get_int("refit.heights") == heights and q.get_int("refit.launches") == launches
        assert q.get_int("stack.entries") == heights + 1 and q.get_int("stack.packed") == 1
        assert q.get_int("stack.in_hbm") == (1 if 256 * 3 * 4 * (heights + 1) > 65536 else 0)
        assert q.get_int("rebuild.launches") == (launches if len(scene.tris) == 1 else 8 + launches)
        assert q.get_int("layout.pairs") == 64 * max(len(scene.tris) - 1, 1)
        if name == "grid":
            assert launches >= 3 and heights > launches - 2  # a per-level launch, and levels left for the fused tail
    hit = check_hits(built, order, hits, oracle)
    assert (occ == hit).all()
    assert hit.sum() >= 100, "the rays must find the mesh"


@pytest.mark.parametrize("name", ["rubik", "grid", "copies", "three", "oob"])
def test_rebuild_then_refit_keeps_the_rebuilt_topology(torch, rubik, cases, name):
    from srt_amd.query import Query

    scene, verts, built, order, rays, _ = cases[name]
    other = RR.wave(verts, 0.4, 1.1)
    want = S.refit_scene(built, other)  # the rebuild's topology, srt_bvh_refit with the refit's vertices
    with Query(scene, refit=True, rebuild=True) as q:
        q.rebuild(verts_dev(torch, verts))
        q.refit(verts_dev(torch, other))
        hits = q.closest(to_dev(torch, rays)).numpy()
        check_structure(q, want, order)
        assert q.get_int("rebuild.count") == 1 and q.get_int("refit.count") == 1
    check_hits(want, order, hits, O.Oracle(want).trace_closest(1, rays))


@pytest.mark.parametrize("name", ["rubik", "grid", "copies", "two"])
def test_no_state_is_carried_between_rebuilds(torch, cases, name):
    from srt_amd.query import Query

    scene, verts, built, order, rays, oracle = cases[name]
    first = RR.wave(scene.verts, 1.5, 0.7)
    with Query(scene, refit=True, rebuild=True) as q, Query(scene, refit=True, rebuild=True) as once:
        q.rebuild(verts_dev(torch, first))
        after_first = q.layout(), q.tri_order()
        q.rebuild(verts_dev(torch, verts))
        once.rebuild(verts)  # the numpy path uploads and synchronises
        for g, w in zip(q.layout(), once.layout()):
            assert g.shape == w.shape and (g == w).all()
        assert (q.tri_order() == once.tri_order()).all()
        check_structure(q, built, order)
        assert q.get_int("rebuild.count") == 2 and once.get_int("rebuild.count") == 1
        for key in ("stack.entries", "stack.in_hbm", "stack.packed", "refit.heights", "refit.launches", "refit.bytes",
                    "rebuild.depth", "rebuild.launches", "layout.pairs", "layout.roots", "layout.tris", "scene.bytes"):
            assert q.get_int(key) == once.get_int(key), key
        if name in ("rubik", "grid"):
            assert not (after_first[1] == order).all()  # (the first set of vertices gave another order)
        check_hits(built, order, q.closest(to_dev(torch, rays)).numpy(), oracle)


def test_surface_and_temporal_objects_stay_valid(torch, cases):
    """Index stability: srt_hit.triangle stays the scene's triangle index, so a Surface and a Temporal object (with
    set_mesh) built from the scene give, on the rebuilt query's hits, bit for bit what they give on the hits of a query
    that was only refit to the same vertices.  Rays that hit two triangles at one distance are dropped on the CPU."""
    from srt_amd.query import Query
    from srt_amd.surface import Surface
    from srt_amd.temporal import Temporal

    scene, verts, built, order, _, _ = cases["rubik"]
    W, H = 64, 63
    frames = [verts, RR.wave(scene.verts, 0.3, 0.9)]
    lo, hi = bounds(S.refit_scene(scene, verts))
    rays = sphere_rays(lo, hi, 4099, 404)
    keep = np.ones(len(rays), bool)
    for v in frames:  # the oracle alone: where the two trees name different triangles, two lie at one distance
        b, o = S.build_lbvh(scene, v)
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
    with Query(scene, refit=True, rebuild=True) as qb, Query(scene, refit=True) as qr, \
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
            assert (surf.shade(dev, hb) == surf.shade(dev, hr)).all()
            acc = np.ones((H, W, 4), np.float32)
            acc[..., :3] = rng.uniform(0, 6, (H, W, 3)).astype(np.float32)
            acc = torch.from_numpy(acc).cuda()
            tb.set_vertices(vd)
            tr.set_vertices(vd)
            a, b = tb.accumulate(acc, 3, hb, cam), tr.accumulate(acc, 3, hr, cam)
            assert (a.view(torch.int32) == b.view(torch.int32)).all(), f"frame {k}"


def test_an_object_without_a_rebuild_is_as_before(torch, cases):
    """Not enabled, and enabled but never rebuilt: the layout, the hits, the launches and what the object holds."""
    from srt_amd.query import Query

    scene, verts, built, order, rays, _ = cases["rubik"]
    rays = rays[:1500]
    with Query(scene) as plain, Query(scene, refit=True) as flagged, Query(scene, refit=True, rebuild=True) as enabled:
        enabled.enable_rebuild()  # a second call is fine
        want = [plain.get_int(k) for k in ("layout.pairs", "layout.roots", "layout.tris", "scene.bytes")]
        ref_hits = None
        for q in (plain, flagged, enabled):
            q.set_bvh_count(1)
            for g, w in zip(q.layout(), plain.layout()):
                assert g.shape == w.shape and (g == w).all()
            hits = q.closest(to_dev(torch, rays))
            ref_hits = hits.raw if ref_hits is None else ref_hits
            assert (hits.raw == ref_hits).all()
            assert q.get_int("launch.blocks") == plain.get_int("launch.blocks") and q.get_int("launch.block") == 256
            assert q.get_int("scratch.bytes") == 256 and q.get_int("stack.in_hbm") == 0
            assert [q.get_int(k) for k in ("layout.pairs", "layout.roots", "layout.tris", "scene.bytes")] == want
            assert (q.tri_order() == np.arange(len(scene.tris))).all()
            assert q.get_int("rebuild.count") == 0 and q.get_int("rebuild.launches") == 0 and q.get_int("rebuild.depth") == 0
        for q in (plain, flagged):
            assert q.get_int("rebuild") == 0 and q.get_int("rebuild.bytes") == 0
        assert enabled.get_int("rebuild") == 1 and enabled.get_int("refit.bytes") == flagged.get_int("refit.bytes")
        assert enabled.get_int("refit.launches") == flagged.get_int("refit.launches")
        # a refit of the enabled object before any rebuild is the flagged object's
        v = verts_dev(torch, verts)
        enabled.refit(v)
        flagged.refit(v)
        for g, w in zip(enabled.layout(), flagged.layout()):
            assert (g == w).all()


def test_argument_errors_enqueue_nothing(torch, rubik, cases):
    from srt_amd import SrtError, _lib
    from srt_amd.query import Query

    scene, verts, built, order, rays, _ = cases["rubik"]
    good = verts_dev(torch, verts)

    def invalid(call, text):
        with pytest.raises(SrtError) as e:
            call()
        assert e.value.code == _lib.SRT_ERR_INVALID and text in str(e.value)

    with Query(scene) as plain:
        invalid(plain.enable_rebuild, "without SRT_QUERY_REFIT")
        invalid(lambda: plain.rebuild(good), "without SRT_QUERY_REFIT")
        assert plain.get_int("rebuild") == 0
    two = S.Scene.from_models([rubik, S.model_from_triangles(RR.grid_triangles(2))])
    with Query(two, refit=True) as q:
        invalid(q.enable_rebuild, "more than one BVH record")
    with pytest.raises(SrtError):
        Query(two, refit=True, rebuild=True)
    one = cases["one"][0]
    bvhs = one.bvhs.copy()
    bvhs[0]["first_index"] = 1
    moved = dataclasses.replace(one, bvhs=bvhs, nodes=np.concatenate([one.nodes, one.nodes]))
    with Query(moved, refit=True) as q:
        invalid(q.enable_rebuild, "first_index")
    with Query(scene, refit=True) as q:
        invalid(lambda: q.rebuild(good), "not enabled")
        q.enable_rebuild()
        before = q.layout()
        n = len(scene.verts)
        for bad in (torch.cat([good, good[:1]]), good[:-1].contiguous()):
            invalid(lambda: q.rebuild(bad), "n_verts differs")
        flat = torch.zeros(8 * n + 1, dtype=torch.float32, device="cuda")
        view = flat[1:].view(n, 8)
        assert view.is_contiguous() and view.data_ptr() % 16 == 4
        invalid(lambda: q.rebuild(view), "16-byte aligned")
        with pytest.raises(ValueError):
            q.rebuild(good.cpu())
        with pytest.raises(ValueError):
            q.rebuild(good.to(torch.float64))
        assert q.get_int("rebuild.count") == 0
        for g, w in zip(q.layout(), before):
            assert g.shape == w.shape and (g == w).all()
        q.rebuild(good)
        assert q.get_int("rebuild.count") == 1
        check_structure(q, built, order)
