"""GPU: the coherence-sorted ray queries (include/srt_query_sort.h, Query.closest(sort=True) / occluded(sort=True)).

A ray's answer does not depend on which lane traced it, so every comparison is bit for bit: the sorted call's records
against the unsorted call's as uint32 words (t and the normals included, so NaNs compare), the device's permutation and
sorted keys against the host mirror srt_ray_order dword for dword, and -- so that nothing rests on the unsorted call
alone -- the sorted hits against the CPU oracle wherever a test has its answer.
"""
import ctypes as C

import numpy as np
import pytest

import rebuild_models_ref as MR
import refit_ref as RR
import special_rays as SR
import srt_amd as S
import test_gpu_rebuild as RT
import test_gpu_rebuild_models as MT
from conftest import OBJECTS
from oracle import pyoracle as O
from test_gpu_queries import INF_T, MISS, _deep_chain, bounds, check_closest, rubik_rays, sphere_rays, to_dev
from test_gpu_special_rays import same_centroid_leaf
from test_ray_order_api import rule_bits

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
def rubik_70001(rubik_scene):
    """Rays for the batch edges, and the oracle's answer for the first 4099 of them."""
    rays = rubik_rays(rubik_scene, 70001)
    return rays, O.Oracle(rubik_scene).trace_closest(1, rays[:4099])[0]


def words(a):
    return np.ascontiguousarray(a).view(np.uint32)


def sorted_equals_unsorted(q, torch, rays, dev=None):
    """closest and occluded both ways on `rays`; the records agree in every dword, and the device's order and keys are
    the host mirror's after each sorted call.  Returns (hits, occluded) of the sorted calls."""
    dev = to_dev(torch, rays) if dev is None else dev
    plain_h, plain_o = q.closest(dev).numpy(), q.occluded(dev).cpu().numpy()
    want_order, want_keys = S.ray_order(rays)
    sorted_h = q.closest(dev, sort=True)
    assert sorted_h.raw.is_cuda and sorted_h.raw.shape == (len(rays), 8) and sorted_h.raw.dtype == torch.int32
    sorted_h = sorted_h.numpy()
    order, keys = q.ray_order()
    assert (order == want_order).all(), f"{(order != want_order).sum()} positions of the order differ"
    assert (keys == want_keys).all()
    sorted_o = q.occluded(dev, sort=True)
    assert sorted_o.dtype == torch.uint8 and sorted_o.shape == (len(rays),)
    sorted_o = sorted_o.cpu().numpy()
    order, keys = q.ray_order()
    assert (order == want_order).all() and (keys == want_keys).all()
    bad = (words(sorted_h).reshape(-1, 8) != words(plain_h).reshape(-1, 8)).any(1)
    assert not bad.any(), f"closest: {bad.sum()} sorted records differ from the unsorted call's (first: ray {np.flatnonzero(bad)[:1]})"
    assert (sorted_o == plain_o).all(), f"occluded: {(sorted_o != plain_o).sum()} rays differ"
    assert (sorted_o == (sorted_h["triangle"] != MISS)).all()
    return sorted_h, sorted_o


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 257, 4099, 70001])
def test_batch_edges_on_rubik(torch, rubik_scene, rubik_70001, n):
    """One wave, one block of the bounds kernel, past it, several claims, and past the sort's single-tile path."""
    from srt_amd.query import Query

    rays = rubik_70001[0][:n].copy()
    with Query(rubik_scene) as q:
        q.set_bvh_count(1)
        assert (q.get_int("sort.origin_bits"), q.get_int("sort.dir_bits")) == rule_bits()
        assert q.get_int("stack.in_hbm") == 0 and q.get_int("stack.packed") == 1
        hits, occ = sorted_equals_unsorted(q, torch, rays)
        assert q.get_int("sort.count") == 2 and q.get_int("sort.launches") == 4
        assert q.get_int("sort.bytes") >= 16 * n + 24
    if n >= 4099:
        order, _ = S.ray_order(rays)
        assert (order != np.arange(n)).mean() > 0.9  # the oracle's rays arrive in no useful order: the sort moves them
    if n == 4099:
        tri_o, _ = check_closest(rubik_scene, 1, rays, hits)  # the sorted hits against the oracle directly
        assert (tri_o == rubik_70001[1]).all() and (occ == (tri_o != MISS)).all()
        assert hits["triangle"][0] == 365  # the reference's KAT ray is still ray 0


@pytest.fixture(scope="module")
def special_sets(rubik_scene):
    return SR.all_families(rubik_scene)


@pytest.mark.parametrize("family", ["special_values", "mixed_wave", "epsilon_t"])
def test_special_values(torch, rubik_scene, special_sets, family):
    """NaN / Inf / 3e38 origins, zero, denormal, infinite and NaN directions, the T_SPECIALS (special_values: one field at
    a time; mixed_wave: beside generic rays in one wave) and finite intersection_distances around the hit (epsilon_t)."""
    from srt_amd.query import Query

    rays, labels = special_sets[family]
    if family == "special_values":
        t = rays["t"][np.char.startswith(labels, "special_values/t#")]
        assert {v.tobytes() for v in t} == {np.float32(v).tobytes() for v in SR.T_SPECIALS}
    if family == "epsilon_t":
        assert (np.isfinite(rays["t"]) & (rays["t"] < 100)).sum() > 100
    with Query(rubik_scene) as q:
        q.set_bvh_count(1)
        hits, occ = sorted_equals_unsorted(q, torch, rays)
    tri_o, _ = check_closest(rubik_scene, 1, rays, hits)
    assert (occ == (tri_o != MISS)).all()


def test_several_records_a_ghost_record_and_a_moved_matrix(torch, rubik):
    """Two models, the second behind a transform, bvh_count past n_bvhs: the ray is read again through L.idx for every
    record.  Then the matrix moves between two sorted calls."""
    from srt_amd.query import Query

    one = S.Scene.from_models([rubik])
    scene = S.Scene.from_models([rubik, S.load_obj(OBJECTS / "Rubik" / "Rubik.obj")])
    n0 = len(one.tris)
    bvh_of = lambda tri: (tri >= n0).astype(np.uint32)  # noqa: E731
    lo, hi = bounds(one)
    shifts = [np.array((-12.0, 2.0, 5.0)), np.array((3.0, -9.0, 1.0))]
    sets = [sphere_rays(lo, hi, 1500, 31)]
    for k, shift in enumerate(shifts):
        sets.append(sphere_rays(lo + shift, hi + shift, 1500, 32 + k))
    sets.append(sphere_rays(lo - 12, hi + 12, 599, 35, spread=1.1))
    rays = np.concatenate(sets)
    with Query(scene) as q:
        q.set_bvh_count(3)  # bvhs[2] is the shader's out-of-bounds (zero) record
        dev = to_dev(torch, rays)
        for k, shift in enumerate(shifts):
            frame = np.eye(4, dtype=np.float32)
            frame[3, :3] = -shift  # world -> model frame of the second cube (glm column 3)
            q.update_model_matrix(1, frame)
            scene.bvhs[1]["frame"] = frame.reshape(16)
            hits, occ = sorted_equals_unsorted(q, torch, rays, dev)
            tri_o, _ = check_closest(scene, 3, rays, hits, bvh_of=bvh_of)
            hit = tri_o != MISS
            assert (hits["bvh"][hit] == 0).sum() > 200 and (hits["bvh"][hit] == 1).sum() > 200
            assert (occ == hit).all()
        assert q.get_int("sort.count") == 4


def _deep_rays(n_chain=200, n=1000):
    rays = np.zeros(n, S.RAY_DTYPE)
    x = np.float32(1.5) ** np.arange(n_chain).astype(np.float32)
    rays["o"][:n_chain, 0] = x                      # across the chain: one ray down onto each triangle
    rays["o"][:n_chain, 2] = np.float32(10.0) * x
    rays["d"][:n_chain] = (0.0, 0.0, -1.0)
    rays["o"][n_chain:] = (-2.0, 0.01, 0.0)        # along the chain, fanned in y
    rays["d"][n_chain:, 0] = 1.0
    rays["d"][n_chain:, 1] = np.linspace(-0.2, 0.2, n - n_chain, dtype=np.float32)
    rays["t"] = INF_T
    return rays


def _instance_scene(name):
    """(scene, rays, in_hbm, packed): the scenes tests/test_gpu_queries.py and tests/test_gpu_special_rays.py use to reach
    the unsorted instances, and the two together for the fourth combination."""
    if name == "deep_chain":
        tris, rays = _deep_chain(), _deep_rays()
        want = (1, 1)
    elif name == "big_leaf":
        tris = same_centroid_leaf()
        want = (0, 0)
        rays = None
    else:
        # the 256 same-centroid triangles, scaled down and moved beside the chain's start: a deep tree with one big leaf
        blob = (same_centroid_leaf().reshape(-1, 3) * np.float32(1.0 / 1024) + np.array((-3.0, 0.0, 0.0), np.float32))
        tris = np.concatenate([_deep_chain(), blob.astype(np.float32).reshape(-1, 9)])
        want = (1, 0)
        rays = None
    scene = S.Scene.from_models([S.model_from_triangles(tris, kd=(0.6, 0.6, 0.6), ks=(0.1, 0.1, 0.1), ns=8.0)])
    if rays is None:
        lo, hi = bounds(scene)
        rays = sphere_rays(lo, hi, 1500, 77, spread=0.9)
        if name == "deep_big_leaf":
            blo, bhi = blob.min(0).astype(np.float64), blob.max(0).astype(np.float64)
            rays = np.concatenate([_deep_rays(), sphere_rays(blo, bhi, 600, 78, spread=0.9)])
    return scene, rays, want


@pytest.mark.parametrize("name", ["deep_chain", "big_leaf", "deep_big_leaf"])
def test_every_new_instance(torch, name):
    """Stacks in HBM, unpacked stack entries, and both (Rubik, everywhere else here, is LDS stacks and packed entries)."""
    from srt_amd.query import Query

    scene, rays, (in_hbm, packed) = _instance_scene(name)
    with Query(scene) as q:
        q.set_bvh_count(1)
        assert (q.get_int("stack.in_hbm"), q.get_int("stack.packed")) == (in_hbm, packed)
        hits, occ = sorted_equals_unsorted(q, torch, rays)
    tri_o, _ = check_closest(scene, 1, rays, hits)
    assert (occ == (tri_o != MISS)).all() and (tri_o != MISS).sum() >= 50


def test_after_a_refit(torch, rubik_scene):
    from srt_amd.query import Query

    verts = RR.wave(rubik_scene.verts)
    moved = S.refit_scene(rubik_scene, verts)
    lo, hi = bounds(moved)
    rays = np.concatenate([sphere_rays(lo, hi, 2500, 41), SR.triangle_rays(moved, 1599, 42)])
    with Query(rubik_scene, refit=True) as q:
        q.set_bvh_count(1)
        q.refit(RT.verts_dev(torch, verts))
        assert q.get_int("refit.count") == 1
        hits, occ = sorted_equals_unsorted(q, torch, rays)
    tri_o, _ = check_closest(moved, 1, rays, hits)
    assert (occ == (tri_o != MISS)).all() and (tri_o != MISS).mean() > 0.3


@pytest.mark.parametrize("max_leaf", [1, 4])
def test_after_a_rebuild(torch, rubik_scene, max_leaf):
    """The remap launch runs after the sorted call too: Hits.triangle is the scene's index."""
    from srt_amd.query import Query

    verts = RR.wave(rubik_scene.verts)
    built, order = S.build_lbvh(rubik_scene, verts, max_leaf=max_leaf)
    rays = RT.scene_rays("grid", built)
    oracle = O.Oracle(built).trace_closest(1, rays)
    with Query(rubik_scene, refit=True, rebuild=True, rebuild_leaf=max_leaf) as q:
        q.set_bvh_count(1)
        q.rebuild(RT.verts_dev(torch, verts))
        assert q.get_int("rebuild.count") == 1 and q.get_int("rebuild.leaf") == max_leaf
        hits, occ = sorted_equals_unsorted(q, torch, rays)
        assert q.get_int("sort.launches") == 4  # the last sorted call was occluded: no remap
        q.closest(to_dev(torch, rays), sort=True)
        assert q.get_int("sort.launches") == 5
    hit = RT.check_hits(built, order, hits, oracle)
    assert (occ == hit).all() and hit.sum() >= 100


def test_after_a_rebuild_of_several_records(torch, rubik):
    from srt_amd.query import Query

    scene, verts = MR.make_scene("two", rubik)
    built, order = S.build_lbvh_models(scene, verts, max_leaf=4)
    rays = MR.rays_of("two", scene, verts)
    oracle = O.Oracle(built).trace_closest(len(built.bvhs), rays)
    with Query(scene, refit=True, rebuild_models=True, rebuild_leaf=4) as q:
        q.rebuild(RT.verts_dev(torch, verts))
        assert q.get_int("rebuild.records") == 2 and q.get_int("rebuild.count") == 1
        hits, occ = sorted_equals_unsorted(q, torch, rays)
    hit = MT.check_hits(built, order, hits, oracle)  # Hits.triangle the scene's index, Hits.bvh the record
    assert (occ == hit).all()


def test_stream_scratch_and_counters(torch, rubik_scene, rubik_70001):
    """Two sorted calls with different rays and different n back to back on a caller's stream, then an unsorted one, one
    synchronisation; the second reuses the first's buffers; nothing is allocated at a steady n."""
    from srt_amd import SrtError, _lib
    from srt_amd.query import HIT_DTYPE, Query

    all_rays = rubik_70001[0]
    a_rays, b_rays = all_rays[:4099].copy(), all_rays[5000:6500][::-1].copy()
    stream = torch.cuda.Stream()
    with Query(rubik_scene, stream=stream) as q:
        q.set_bvh_count(1)
        assert q.get_int("sort.bytes") == 0 and q.get_int("sort.count") == 0 and q.get_int("sort.launches") == 0
        with pytest.raises(SrtError) as e:
            q.ray_order()
        assert e.value.code == _lib.SRT_ERR_STATE
        with torch.cuda.stream(stream):
            a_dev, b_dev = to_dev(torch, a_rays), to_dev(torch, b_rays)
            a = q.closest(a_dev, sort=True)
            b = q.closest(b_dev, sort=True)
            c = q.closest(a_dev)
            b_occ = q.occluded(b_dev, sort=True)
        stream.synchronize()
        ha, hb, hc, ob = a.numpy(), b.numpy(), c.numpy(), b_occ.cpu().numpy()
        stream.synchronize()
        tri_a, _ = check_closest(rubik_scene, 1, a_rays, ha)
        tri_b, _ = check_closest(rubik_scene, 1, b_rays, hb)
        assert (words(ha) == words(hc)).all() and (ob == (tri_b != MISS)).all()
        assert (tri_a == rubik_70001[1]).all()
        order, keys = q.ray_order()  # of the last sorted call: b's
        want_order, want_keys = S.ray_order(b_rays)
        assert len(order) == 1500 and (order == want_order).all() and (keys == want_keys).all()
        assert q.get_int("sort.count") == 3 and q.get_int("sort.launches") == 4
        held = q.get_int("sort.bytes")
        assert held >= 16 * 4099 + 24  # the smaller calls ran in the first call's buffers
        # n differs from the last sorted call's
        buf = np.zeros(4099, np.uint32)
        assert _lib.lib().srt_query_copy_ray_order(q.handle, S._ptr(buf), None, 4099) == _lib.SRT_ERR_STATE
        # a repeat at the same n into caller-owned tensors: no torch allocation, no growth of the library's scratch
        out = torch.empty((4099, 8), dtype=torch.int32, device="cuda")
        mem = torch.cuda.memory_allocated()
        rc = _lib.lib().srt_query_closest_sorted(q.handle, C.c_void_p(a_dev.data_ptr()), 4099, C.c_void_p(out.data_ptr()))
        stream.synchronize()
        assert rc == _lib.SRT_OK and torch.cuda.memory_allocated() == mem and q.get_int("sort.bytes") == held
        assert (words(out.cpu().numpy().view(HIT_DTYPE).reshape(-1)) == words(ha)).all()
        assert q.get_int("sort.count") == 4
        # n == 0 launches nothing and counts nothing; bad pointers fail as the unsorted calls fail
        lib, h = _lib.lib(), q.handle
        assert lib.srt_query_closest_sorted(h, None, 0, None) == _lib.SRT_OK
        assert lib.srt_query_occluded_sorted(h, None, 0, None) == _lib.SRT_OK
        assert q.get_int("sort.count") == 4 and q.get_int("sort.bytes") == held
        assert lib.srt_query_closest_sorted(h, None, 4, C.c_void_p(out.data_ptr())) == _lib.SRT_ERR_INVALID
        assert lib.srt_query_closest_sorted(h, C.c_void_p(a_dev.data_ptr()), 4, None) == _lib.SRT_ERR_INVALID
        assert lib.srt_query_closest_sorted(h, C.c_void_p(a_dev.data_ptr() + 4), 4, C.c_void_p(out.data_ptr())) == _lib.SRT_ERR_INVALID
        assert lib.srt_query_closest_sorted(h, C.c_void_p(a_dev.data_ptr()), 4, C.c_void_p(out.data_ptr() + 4)) == _lib.SRT_ERR_INVALID
        assert lib.srt_query_occluded_sorted(h, C.c_void_p(a_dev.data_ptr() + 8), 4, C.c_void_p(out.data_ptr())) == _lib.SRT_ERR_INVALID
        assert lib.srt_query_closest_sorted(h, C.c_void_p(a_dev.data_ptr()), 0x80000000, C.c_void_p(out.data_ptr())) == _lib.SRT_ERR_INVALID
        assert q.get_int("sort.count") == 4
        # the refused calls left the last call's state alone
        assert lib.srt_query_copy_ray_order(h, S._ptr(buf), None, 4099) == _lib.SRT_OK
        assert (buf == S.ray_order(a_rays)[0]).all()
    # the default stream mode: ordered with torch's current stream by events
    with Query(rubik_scene) as q:
        q.set_bvh_count(1)
        dev = to_dev(torch, a_rays)
        hd = q.closest(dev, sort=True).numpy()
        assert (words(hd) == words(ha)).all()


def test_numpy_path_equals_the_tensor_path(torch, rubik_scene, rubik_70001):
    from srt_amd.query import HIT_DTYPE, Query

    rays = rubik_70001[0][:4099].copy()
    with Query(rubik_scene) as q:
        q.set_bvh_count(1)
        hn = q.closest(rays, sort=True)
        on = q.occluded(rays, sort=True)
        assert isinstance(hn, np.ndarray) and hn.dtype == HIT_DTYPE and isinstance(on, np.ndarray)
        dev = to_dev(torch, rays)
        ht = q.closest(dev, sort=True).numpy()
        ot = q.occluded(dev, sort=True).cpu().numpy()
        plain = q.closest(rays)
    assert (words(hn) == words(ht)).all() and (on == ot).all() and (words(hn) == words(plain)).all()
    assert (rubik_70001[1] == hn["triangle"]).all()
