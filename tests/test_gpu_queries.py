"""GPU: the ray-query service (include/srt_query.h, srt_amd.query.Query) vs the CPU oracle, bit for bit.

Every field of srt_hit is compared with O.Oracle(scene).trace_closest: `==` on the integers, bits_equal on t
and on the normal (which no other GPU test compares).  Rays and results are torch device tensors unless a
test says otherwise.
"""
import ctypes as C

import numpy as np
import pytest

import srt_amd as S
from srt_amd import render as R
from conftest import OBJECTS, bits_equal, oracle_render
from oracle import pyoracle as O

pytestmark = pytest.mark.gpu

MISS = 0xFFFFFFFF
INF_T = np.float32(1e30)


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


def bounds(scene):
    p = scene.verts["pos"]
    return p.min(0).astype(np.float64), p.max(0).astype(np.float64)


def sphere_rays(lo, hi, n, seed, spread=1.7):
    """Origins on a sphere around the box [lo, hi] (radius: twice its diagonal), directions towards points
    jittered inside the box scaled by `spread` about its centre (so some rays pass beside the model)."""
    rng = np.random.default_rng(seed)
    c, half = (lo + hi) / 2, (hi - lo) / 2
    v = rng.normal(size=(n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    rays = np.zeros(n, S.RAY_DTYPE)
    rays["o"] = (c + 2.0 * np.linalg.norm(hi - lo) * v).astype(np.float32)
    tgt = c + rng.uniform(-1, 1, size=(n, 3)) * half * spread
    rays["d"] = (tgt - rays["o"].astype(np.float64)).astype(np.float32)
    rays["t"] = INF_T
    return rays


def rubik_rays(scene, n, seed=2025):
    """The reference's two KAT rays first, then sphere_rays."""
    from test_oracle_pins import kat_rays

    lo, hi = bounds(scene)
    k = min(n, 2)
    return np.concatenate([kat_rays(2)[::-1][:k], sphere_rays(lo, hi, n - k, seed)])


def to_dev(torch, rays):
    return torch.from_numpy(rays.view(np.float32).reshape(-1, 8).copy()).cuda()


def check_closest(scene, bvh_count, rays, hits, *, bvh_of=None):
    """`hits`: HIT_DTYPE records from the library; every field against the oracle."""
    tri_o, t_o, n_o, st = O.Oracle(scene).trace_closest(bvh_count, rays)
    assert st["stack_overflow"] == 0  # (the oracle's own 64-entry stack: the inputs stay inside it)
    assert (hits["triangle"] == tri_o).all(), f"{(hits['triangle'] != tri_o).sum()} triangles differ"
    assert bits_equal(hits["t"], t_o).all()
    assert bits_equal(hits["normal"], n_o).all()
    hit = tri_o != MISS
    assert (hits["material"][hit] == scene.tris["mat"][tri_o[hit]]).all()
    if bvh_of is None:
        assert (hits["bvh"] == 0).all()
    else:
        assert (hits["bvh"][hit] == bvh_of(tri_o[hit])).all()
    # the miss record: all-ones triangle, the input distance, zero normal, material and bvh
    miss = ~hit
    assert bits_equal(hits["t"][miss], rays["t"][miss]).all()
    assert (hits["normal"][miss].view(np.uint32) == 0).all()
    assert (hits["material"][miss] == 0).all() and (hits["bvh"][miss] == 0).all() and (hits["pad"] == 0).all()
    return tri_o, t_o


@pytest.fixture(scope="module")
def rubik_4099(rubik_scene):
    rays = rubik_rays(rubik_scene, 4099)
    tri_o, _, _, _ = O.Oracle(rubik_scene).trace_closest(1, rays)
    return rays, tri_o


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 257, 4099])
def test_batch_edges_on_rubik(torch, rubik_scene, rubik_4099, n):
    """Ray counts around the 64-ray batch and the 256-lane block, and one that takes several claims."""
    from srt_amd.query import Query

    rays = rubik_4099[0][:n].copy()
    if n == 4099:
        hit = rubik_4099[1] != MISS
        assert hit.mean() >= 0.25 and (~hit).mean() >= 0.10  # the oracle alone: the set exercises both
    with Query(rubik_scene) as q:
        q.set_bvh_count(1)
        assert q.get_int("stack.in_hbm") == 0 and q.get_int("launch.block") == 256
        h = q.closest(to_dev(torch, rays))
        assert h.raw.is_cuda and h.raw.shape == (n, 8) and h.raw.dtype == torch.int32
        hits = h.numpy()
        check_closest(rubik_scene, 1, rays, hits)
        assert hits["triangle"][0] == 365  # the reference's KAT: loader triangle 17 in BVH order
        # the accessors view the same storage
        assert (h.triangle.cpu().numpy().view(np.uint32) == hits["triangle"]).all()
        assert bits_equal(h.t.cpu().numpy(), hits["t"]).all()
        assert bits_equal(h.normal.cpu().numpy(), hits["normal"]).all()
        assert (h.hit.cpu().numpy() == (hits["triangle"] != MISS)).all()


def test_finite_tmax_and_occlusion(torch, rubik_scene):
    """intersection_distance just under, at, and just over the closest hit, and infinite; plus missing rays.
    The exact-t group is the strict `<` edge (it may still hit a farther tie: the oracle decides)."""
    from srt_amd.query import Query

    cand = rubik_rays(rubik_scene, 12000, seed=7)
    tri, t, _, _ = O.Oracle(rubik_scene).trace_closest(1, cand)
    hit_i, miss_i = np.flatnonzero(tri != MISS)[:2048], np.flatnonzero(tri == MISS)[:512]
    assert len(hit_i) == 2048 and len(miss_i) == 512
    groups = []
    for tmax in (np.nextafter(t[hit_i], np.float32(0)), t[hit_i], np.nextafter(t[hit_i], np.float32(np.inf)),
                 np.full(2048, np.inf, np.float32)):
        g = cand[hit_i].copy()
        g["t"] = tmax
        groups.append(g)
    rays = np.concatenate(groups + [cand[miss_i]])
    with Query(rubik_scene) as q:
        q.set_bvh_count(1)
        dev = to_dev(torch, rays)
        hits = q.closest(dev).numpy()
        occ = q.occluded(dev)
        assert occ.is_cuda and occ.dtype == torch.uint8 and occ.shape == (len(rays),)
        occ = occ.cpu().numpy()
    tri_o, _ = check_closest(rubik_scene, 1, rays, hits)
    assert (occ == (tri_o != MISS)).all()
    assert (occ == (hits["triangle"] != MISS)).all()
    # the oracle alone: just under t (and at t) that triangle is no longer accepted; one ulp over t most rays
    # find it again (not all: a box's entry distance may round above the triangle's own t); infinity finds all
    assert (tri_o[:4096] != np.tile(tri[hit_i], 2)).all()
    assert 0.5 < (tri_o[4096:6144] == tri[hit_i]).mean() < 1.0
    assert (tri_o[6144:8192] == tri[hit_i]).all() and (tri_o[-512:] == MISS).all()


def test_two_models_transform_and_ghost_record(torch, rubik):
    from srt_amd.query import Query
    from test_oracle_pins import kat_rays

    second = S.load_obj(OBJECTS / "Rubik" / "Rubik.obj")
    scene = S.Scene.from_models([rubik, second])
    n0 = len(S.Scene.from_models([rubik]).tris)
    frame = np.eye(4, dtype=np.float32)
    frame[3, :3] = (12.0, -2.0, -5.0)  # world -> model frame of the second cube (glm column 3)
    lo, hi = bounds(S.Scene.from_models([rubik]))
    shift = np.array((-12.0, 2.0, 5.0))
    rays = np.concatenate([sphere_rays(lo, hi, 1500, 31), sphere_rays(lo + shift, hi + shift, 1500, 32),
                           sphere_rays(np.minimum(lo, lo + shift), np.maximum(hi, hi + shift), 1099, 33, spread=1.1)])
    with Query(scene) as q:
        q.update_model_matrix(1, frame)
        q.set_bvh_count(3)  # bvhs[2] is the shader's out-of-bounds (zero) record
        scene.bvhs[1]["frame"] = frame.reshape(16)
        dev = to_dev(torch, rays)
        hits = q.closest(dev).numpy()
        tri_o, _ = check_closest(scene, 3, rays, hits, bvh_of=lambda tri: (tri >= n0).astype(np.uint32))
        hit = tri_o != MISS
        assert (hits["bvh"][hit] == 0).sum() > 300 and (hits["bvh"][hit] == 1).sum() > 300
        assert (q.occluded(dev).cpu().numpy() == hit).all()
        # the KAT's "every ray misses" matrix (BVH_intergration_tests.cpp:96-113), on both records
        m = np.zeros((4, 4), np.float32)
        for i in range(4):
            m[i, i] = 0.000001
        m[0, 3], m[1, 3], m[2, 3] = 10, 1000, 10
        for b in range(2):
            q.update_model_matrix(b, m)
            scene.bvhs[b]["frame"] = m.reshape(16)
        kr = kat_rays(64)
        hits = q.closest(to_dev(torch, kr)).numpy()
        check_closest(scene, 3, kr, hits, bvh_of=lambda tri: (tri >= n0).astype(np.uint32))
        assert (hits["triangle"] == MISS).all()


def _deep_chain(n=200):
    """Triangles at x = 1.5^k: the midpoint split peels one or two off per level, so the tree is about
    n / 1.5 levels deep -- beyond what the LDS stacks hold."""
    tri = []
    for k in range(n):
        x, s = np.float32(1.5) ** k, np.float32(0.3) * np.float32(1.5) ** k
        tri.append([[x - s, -s, 0.0], [x + s, -s, 0.0], [x, s, 0.0]])
    return np.asarray(tri, np.float32).reshape(-1, 9)


def test_deep_tree_stacks_in_hbm(torch):
    from srt_amd.query import Query

    model = S.model_from_triangles(_deep_chain(), kd=(0.6, 0.6, 0.6), ks=(0.1, 0.1, 0.1), ns=8.0)
    depth = model.info()["max_depth"]
    assert depth > 90
    scene = S.Scene.from_models([model])
    n = 200
    rays = np.zeros(1000, S.RAY_DTYPE)
    x = np.float32(1.5) ** np.arange(n).astype(np.float32)
    rays["o"][:n, 0] = x                      # across the chain: one ray down onto each triangle
    rays["o"][:n, 2] = np.float32(10.0) * x
    rays["d"][:n] = (0.0, 0.0, -1.0)
    rays["o"][n:] = (-2.0, 0.01, 0.0)        # along the chain, fanned in y
    rays["d"][n:, 0] = 1.0
    rays["d"][n:, 1] = np.linspace(-0.2, 0.2, 1000 - n, dtype=np.float32)
    rays["t"] = INF_T
    with Query(scene) as q:
        q.set_bvh_count(1)
        assert q.get_int("stack.in_hbm") == 1 and q.get_int("stack.entries") == depth + 1
        dev = to_dev(torch, rays)
        hits = q.closest(dev).numpy()
        occ = q.occluded(dev).cpu().numpy()
        assert q.get_int("scratch.bytes") > 4 * 256 * 2 * (depth + 1)
    tri_o, _ = check_closest(scene, 1, rays, hits)
    assert (tri_o[:60] != MISS).all()
    assert (occ == (tri_o != MISS)).all()


def _coincident_obj(tmp_path):
    """A floor (y = 0) and a back wall (z = -6), each a 4x4 grid of quads written three times: 'red' and
    'green' are the same triangles (twins in one leaf), 'blue' is the grid shifted by half a cell in the same
    plane.  Every hit on them is a distance tie that only the visit order settles (`t <` is strict)."""
    (tmp_path / "m.mtl").write_text("newmtl red\nKd 0.9 0.1 0.1\nKs 0.2 0.2 0.2\nNs 20\n"
                                    "newmtl green\nKd 0.1 0.9 0.1\nKs 0.5 0.5 0.5\nNs 80\n"
                                    "newmtl blue\nKd 0.1 0.1 0.9\nKs 0.05 0.05 0.05\nNs 5\n")
    lines, nv = ["mtllib m.mtl"], 0

    def grid(corner, du, dv, n=4):
        nonlocal nv
        base = nv
        for j in range(n + 1):
            for i in range(n + 1):
                p = np.asarray(corner, np.float64) + i * np.asarray(du) + j * np.asarray(dv)
                lines.append("v %.6g %.6g %.6g" % tuple(p))
                nv += 1
        return [(base + j * (n + 1) + i + 1, base + j * (n + 1) + i + 2, base + (j + 1) * (n + 1) + i + 2,
                 base + (j + 1) * (n + 1) + i + 1) for j in range(n) for i in range(n)]

    floor = grid((-8, 0, -8), (4, 0, 0), (0, 0, 4))
    wall = grid((-8, 0, -6), (4, 0, 0), (0, 3.5, 0))
    floor_b = grid((-6, 0, -6), (4, 0, 0), (0, 0, 4))
    wall_b = grid((-6, 1.75, -6), (4, 0, 0), (0, 3.5, 0))
    for mtl, quads in (("red", floor + wall), ("green", floor + wall), ("blue", floor_b + wall_b)):
        lines.append("usemtl " + mtl)
        lines += ["f %d %d %d %d" % q for q in quads]
    (tmp_path / "m.obj").write_text("\n".join(lines) + "\n")
    return tmp_path / "m.obj"


def test_ties_keep_the_first_visited(torch, tmp_path):
    from srt_amd.query import Query

    scene = S.Scene.from_models([S.load_obj(_coincident_obj(tmp_path))])
    assert len(scene.tris) == 3 * 2 * 32
    rng = np.random.default_rng(17)
    n = 4096
    rays = np.zeros(n, S.RAY_DTYPE)
    rays["o"] = rng.uniform([-7, 0.5, -5], [7, 12, 6], size=(n, 3)).astype(np.float32)
    tgt = np.where((np.arange(n) % 2 == 0)[:, None],
                   np.stack([rng.uniform(-7, 7, n), np.zeros(n), rng.uniform(-7, 7, n)], 1),      # the floor
                   np.stack([rng.uniform(-7, 7, n), rng.uniform(0, 13, n), np.full(n, -6.0)], 1))  # the wall
    rays["d"] = (tgt - rays["o"]).astype(np.float32)
    rays["t"] = INF_T
    with Query(scene) as q:
        q.set_bvh_count(1)
        hits = q.closest(to_dev(torch, rays)).numpy()
    tri_o, _ = check_closest(scene, 1, rays, hits)
    hit = tri_o != MISS
    assert hit.mean() > 0.95
    # twins: a hit on either is a tie by construction, and the material tells which one won
    corners = scene.verts["pos"][scene.tris["v"]].reshape(len(scene.tris), 9)
    keys = [c.tobytes() for c in corners]
    twinned = np.array([keys.count(k) > 1 for k in keys])
    assert twinned[tri_o[hit]].mean() > 0.3


def test_mesh_past_lds_size_incoherent_rays(torch):
    """4,096 triangles; half the rays start on the surface in random directions (the incoherent case the
    refill is for: neighbouring lanes finish at very different times)."""
    from srt_amd.query import Query

    scene = S.Scene.from_models([R.torus_knot_model(64, 32)])
    assert len(scene.tris) == 4096
    lo, hi = bounds(scene)
    rng = np.random.default_rng(99)
    n = 4096
    surf = np.zeros(n, S.RAY_DTYPE)
    corners = scene.verts["pos"][scene.tris["v"][rng.integers(0, len(scene.tris), n)]].astype(np.float64)
    w = rng.dirichlet((1, 1, 1), n)
    surf["o"] = (corners * w[:, :, None]).sum(1).astype(np.float32)
    d = rng.normal(size=(n, 3))
    surf["d"] = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    surf["t"] = INF_T
    rays = np.concatenate([sphere_rays(lo, hi, n, 5), surf])
    with Query(scene) as q:
        q.set_bvh_count(1)
        dev = to_dev(torch, rays)
        hits = q.closest(dev).numpy()
        occ = q.occluded(dev).cpu().numpy()
    tri_o, _ = check_closest(scene, 1, rays, hits)
    assert (occ == (tri_o != MISS)).all()
    assert 0.2 < (tri_o[n:] != MISS).mean() < 0.999


def test_stream_scratch_and_coexistence_with_a_renderer(torch, rubik, rubik_scene, rubik_4099):
    """Two calls enqueued back to back on a non-default torch stream, one synchronize; a smaller call
    allocates nothing; and a Renderer in the same process still matches the oracle afterwards."""
    from srt_amd import _lib
    from srt_amd.query import HIT_DTYPE, Query

    rays = rubik_4099[0]
    stream = torch.cuda.Stream()
    with Query(rubik_scene, stream=stream) as q:
        q.set_bvh_count(1)
        assert q.get_int("bvh_count") == 1
        with torch.cuda.stream(stream):
            dev = to_dev(torch, rays)
            a = q.closest(dev)
            b = q.occluded(dev)
            c = q.closest(dev[:1000])
        stream.synchronize()
        ha, hb, hc = a.numpy(), b.cpu().numpy(), c.numpy()
        stream.synchronize()
        with torch.cuda.stream(stream):
            sa = q.closest(dev).numpy()
            sb = q.occluded(dev).cpu().numpy()
        assert (ha.view(np.uint32) == sa.view(np.uint32)).all() and (hb == sb).all()
        assert (hc.view(np.uint32) == ha[:1000].view(np.uint32)).all()
        check_closest(rubik_scene, 1, rays, ha)
        # a smaller call into caller-owned tensors: no torch allocation, no growth of the library's scratch
        out = torch.empty((len(rays), 8), dtype=torch.int32, device="cuda")
        scratch, mem = q.get_int("scratch.bytes"), torch.cuda.memory_allocated()
        rc = _lib.lib().srt_query_closest(q.handle, C.c_void_p(dev.data_ptr()), 129, C.c_void_p(out.data_ptr()))
        stream.synchronize()
        assert rc == _lib.SRT_OK
        assert torch.cuda.memory_allocated() == mem and q.get_int("scratch.bytes") == scratch
        assert (out[:129].cpu().numpy().view(HIT_DTYPE).reshape(-1).view(np.uint32) == ha[:129].view(np.uint32)).all()
        assert q.get_int("launch.blocks") == 1
        # n == 0 launches nothing
        assert _lib.lib().srt_query_closest(q.handle, None, 0, None) == _lib.SRT_OK
        setup = R.make_setup(64, 64, show_model=True, models=[rubik])
        rdr = R.Renderer(setup, device=0)
        try:
            rdr.render(2, count=True)
            rdr.finish()
            acc, outp = rdr.accum(), rdr.output()
        finally:
            rdr.close()
        want_acc, want_out, _ = oracle_render(setup, 2)
        assert bits_equal(acc, want_acc).all() and (outp == want_out).all()
        # and the query object is undisturbed by the render
        with torch.cuda.stream(stream):
            again = q.closest(dev).numpy()
        assert (again.view(np.uint32) == ha.view(np.uint32)).all()


def test_numpy_path_equals_the_tensor_path(torch, rubik_scene, rubik_4099):
    from srt_amd.query import HIT_DTYPE, Query

    rays = rubik_4099[0]
    with Query(rubik_scene) as q:
        q.set_bvh_count(1)
        hn = q.closest(rays)
        on = q.occluded(rays)
        assert isinstance(hn, np.ndarray) and hn.dtype == HIT_DTYPE and isinstance(on, np.ndarray)
        dev = to_dev(torch, rays)
        ht = q.closest(dev).numpy()
        ot = q.occluded(dev).cpu().numpy()
    assert (hn.view(np.uint32) == ht.view(np.uint32)).all() and (on == ot).all()
    assert (rubik_4099[1] == hn["triangle"]).all()
