"""GPU: temporal reprojection that follows moving models (include/srt_temporal_motion.h, Temporal.set_models)
against the independent numpy float32 restatement (tests/temporal_motion_ref.py, which never calls into the
library): rgb bit for bit (bits_equal treats any NaN as equal to any NaN) and N exactly, after every frame.

The Rubik references (oracle hits per pose, the oracle's 256-spp frame of the last pose) are computed once per
module and left unchanged.
"""
import copy
import ctypes as C

import numpy as np
import pytest

import denoise_ref as D
import srt_amd as S
import temporal_motion_ref as M
import temporal_ref as T
from srt_amd import render as R
from conftest import OBJECTS, bits_equal, oracle_render
from oracle import pyoracle as O

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (5, 1), (37, 23), (70, 41)]
CHUNK = 32  # SRT_TEMPORAL_MODELS_PER_LAUNCH: "launches" is 1 + ceil(n / 32) while poses are set


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


def hit_records(tri, t, n, bvh):
    from srt_amd.query import HIT_DTYPE

    hits = np.zeros(tri.size, HIT_DTYPE)
    hits["triangle"], hits["t"], hits["normal"], hits["bvh"] = tri.reshape(-1), t.reshape(-1), n.reshape(-1, 3), bvh.reshape(-1)
    return hits


def to_dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def hits_dev(torch, hits):
    return torch.from_numpy(hits.view(np.int32).reshape(-1, 8).copy()).cuda()


def set_both(tp, ref, poses):
    tp.set_models([p[0] for p in poses], [p[1] for p in poses])
    ref.set_models(poses)


def step(torch, tp, ref, cam, accum, fields, frames=3):
    """One frame through the GPU object and the restatement; asserts they agree and returns the restatement's."""
    got = tp.accumulate(to_dev(torch, accum), frames, hits_dev(torch, hit_records(*fields)), cam)
    tp.synchronize()
    got = got.cpu().numpy()
    want = ref.accumulate(accum, frames, D.make_guide(*fields), cam)
    bad = int((~bits_equal(got[..., :3], want[..., :3])).sum()), int((got[..., 3] != want[..., 3]).sum())
    print(f"frame {ref.frames - 1}: {bad[0]} colour components and {bad[1]} history lengths differ")
    assert bad == (0, 0)
    assert tp.get_int("launches") == 1 + -(-len(ref.Q) // CHUNK) and tp.get_int("models") == len(ref.Q)
    return want


@pytest.mark.parametrize("w,h", SIZES)
def test_two_wall_scene_bit_exact(torch, w, h):
    """1x1, 5x1, 37x23 and 70x41: five frames of the two-wall scene in which the square stands, translates twice and
    then turns about z under a non-uniform scale while the camera makes its small moves, the GPU equal to the
    restatement after every frame.  On the restatement alone (CPU): from 37 wide the last frame both reuses and
    rejects, the moved square uncovering wall that has no history -- at 37x23 0.949 of the hit pixels reuse and 0.051
    are rejected with 0.589 of the image a miss, at 70x41 0.946, 0.054 and 0.590 -- and the poses change the result
    (at 70x41 every pixel of the square reuses; without poses 0.934 of them would)."""
    from srt_amd.temporal import Temporal

    ref, plain = M.TemporalMotionRef(w, h), T.TemporalRef(w, h)
    with Temporal(w, h) as tp:
        for cam, accum, fields, poses in M.moving_two_wall_frames(w, h):
            set_both(tp, ref, poses)
            moving = ref.motion()[0]
            res = step(torch, tp, ref, cam, accum, fields)
            res_plain = plain.accumulate(accum, 3, D.make_guide(*fields), cam)
        assert tp.get_int("frames") == 5 and tp.get_int("history") == 1 and tp.get_int("models.bytes") == 128
    assert moving.tolist() == [False, True]
    if w >= 37:
        hit, square = fields[0] != D.MISS, (fields[0] != D.MISS) & (fields[3] == 1)
        n4 = res[..., 3][hit]
        print(f"frame 4: {(n4 >= 2).mean():.3f} of hit pixels reuse, {(n4 == 1).mean():.3f} rejected, {(~hit).mean():.3f} miss; "
              f"of the square's {int(square.sum())} pixels {(res[..., 3][square] >= 2).mean():.3f} reuse, "
              f"{(res_plain[..., 3][square] >= 2).mean():.3f} without poses")
        assert (n4 >= 2).mean() >= 0.5 and (n4 == 1).mean() >= 0.02 and (~hit).mean() >= 0.10
        assert (res[..., 3][~hit] == 1).all()
        assert (res[..., 3][square] >= 2).all() and not bits_equal(res[square], res_plain[square]).all()


def test_constant_poses_equal_no_poses(torch):
    """37x23, three cameras: an object whose poses never change (the square turned and scaled, stated again before
    every frame) gives, bit for bit, what an object without poses gives."""
    from srt_amd.temporal import Temporal

    w, h = 37, 23
    tilted = M.pose_from_model(M.column_major(M.rotation("z", 10.0) @ np.diag([1.1, 0.9, 1.0]), (.2, .05, .1)))
    poses = [M.pose_from_model(M.IDENTITY), tilted]
    rng = np.random.default_rng(21)
    ref = M.TemporalMotionRef(w, h)
    with Temporal(w, h) as posed, Temporal(w, h) as bare:
        for pos, yaw, pitch in M.CAMERAS[1:4]:
            cam = T.camera_vectors(pos, yaw, pitch)
            fields = M.posed_two_wall_guide(cam, w, h, [p[0] for p in poses])[:4]
            accum = np.ones((h, w, 4), np.float32)
            accum[..., :3] = rng.uniform(0, 6, (h, w, 3)).astype(np.float32)
            set_both(posed, ref, poses)
            want = step(torch, posed, ref, cam, accum, fields)
            got = bare.accumulate(to_dev(torch, accum), 3, hits_dev(torch, hit_records(*fields)), cam)
            bare.synchronize()
            assert bits_equal(got.cpu().numpy(), want).all()
            assert posed.get_int("launches") == 2 and bare.get_int("launches") == 1
    assert (want[..., 3] >= 2).mean() > 0.2


def test_seventy_records_ids_and_launches(torch):
    """37x23, 70 records (three upload launches): the guide's `bvh` is overwritten in stripes of 6 pixels with the ids
    0..70 in turn, every record moved by its own small translation between frames.  Id 70 is past the poses (the
    static fallback) and the miss pixels stay, so the miss id is met too; launches == 1 + ceil(70 / 32) == 4."""
    from srt_amd.temporal import Temporal

    w, h, n = 37, 23, 70
    stripes = (np.arange(w * h, dtype=np.uint32) // 6 % (n + 1)).reshape(h, w)
    assert stripes.max() == n and set(np.unique(stripes)) == set(range(n + 1))

    def poses(k):
        return [M.pose_from_model(M.column_major(translation=(1e-3 * k * (r + 1), -5e-4 * k * r, 2e-3 * k * (r % 5))))
                for r in range(n)]

    ref, plain = M.TemporalMotionRef(w, h), T.TemporalRef(w, h)
    rng = np.random.default_rng(33)
    with Temporal(w, h) as tp:
        for k, (pos, yaw, pitch) in enumerate(M.CAMERAS[:3]):
            cam = T.camera_vectors(pos, yaw, pitch)
            tri, t, nrm, _ = T.two_wall_guide(cam, w, h)
            assert (tri == D.MISS).sum() > 100
            fields = (tri, t, nrm, stripes)
            accum = np.ones((h, w, 4), np.float32)
            accum[..., :3] = rng.uniform(0, 6, (h, w, 3)).astype(np.float32)
            set_both(tp, ref, poses(k))
            moving = ref.motion()[0]
            want = step(torch, tp, ref, cam, accum, fields)
            want_plain = plain.accumulate(accum, 3, D.make_guide(*fields), cam)
            assert tp.get_int("launches") == 4 and tp.get_int("models.bytes") == 64 * n
            if k:
                assert moving.all()
                last = (stripes == n) & (tri != D.MISS)  # past the poses: as if static
                assert last.sum() >= 4 and bits_equal(want[last], want_plain[last]).all()
                assert not bits_equal(want, want_plain).all()
    assert (want[..., 3] >= 2).mean() > 0.2


def test_lifecycle(torch):
    """Poses first stated after frame 0 are static for one frame and move from the next; reset keeps the poses and
    drops the previous ones; n == 0 restores the static kernel and one launch; only a larger n changes models.bytes;
    accumulate allocates nothing."""
    from srt_amd import _lib
    from srt_amd.temporal import Temporal

    w, h = 37, 23
    still = M.pose_from_model(M.IDENTITY)

    def at(x):
        return [still, M.pose_from_model(M.column_major(translation=(x, 0.02, 0)))]

    cam = T.camera_vectors(*M.CAMERAS[0])
    rng = np.random.default_rng(41)
    ref = M.TemporalMotionRef(w, h)

    def frame(tp, poses):
        fields = M.posed_two_wall_guide(cam, w, h, [p[0] for p in poses] if poses else (M.IDENTITY, M.IDENTITY))[:4]
        accum = np.ones((h, w, 4), np.float32)
        accum[..., :3] = rng.uniform(0, 6, (h, w, 3)).astype(np.float32)
        moving = ref.motion()[0].tolist()
        return moving, step(torch, tp, ref, cam, accum, fields), fields

    with Temporal(w, h) as tp:
        assert tp.get_int("models") == 0 and tp.get_int("models.bytes") == 0
        assert frame(tp, None)[0] == [] and tp.get_int("launches") == 1
        set_both(tp, ref, at(0.1))
        assert tp.get_int("models.bytes") == 128 and tp.get_int("scratch.bytes") == 72 * w * h
        moving, out, fields = frame(tp, at(0.1))
        assert moving == [False, False] and tp.get_int("launches") == 2  # first stated after the previous frame
        set_both(tp, ref, at(0.2))
        moving, out, fields = frame(tp, at(0.2))
        square = M.interior((fields[3] == 1) & (fields[0] != D.MISS))
        assert moving == [False, True] and square.sum() > 10 and (out[..., 3][square] >= 2).all()  # followed: 2 or 3
        tp.reset()
        ref.reset()
        assert tp.get_int("models") == 2 and tp.get_int("history") == 0
        set_both(tp, ref, at(0.3))
        moving, out, _ = frame(tp, at(0.3))
        assert moving == [False, False] and (out[..., 3] == 1).all() and tp.get_int("launches") == 2
        set_both(tp, ref, at(0.4))
        moving, out, fields = frame(tp, at(0.4))
        square = M.interior((fields[3] == 1) & (fields[0] != D.MISS))
        assert moving == [False, True] and (out[..., 3][square] == 2).all()
        set_both(tp, ref, [])
        assert tp.get_int("models") == 0 and tp.get_int("models.bytes") == 128
        assert frame(tp, None)[0] == [] and tp.get_int("launches") == 1
        for n, want in ((2, 128), (1, 128), (3, 192), (2, 192), (0, 192), (3, 192), (5, 320)):
            tp.set_models([M.IDENTITY] * n, [M.IDENTITY] * n)
            assert tp.get_int("models.bytes") == want and tp.get_int("models") == n
        # a raw call with everything allocated beforehand: accumulate itself allocates nothing
        set_both(tp, ref, at(0.5) + [still])
        fields = M.posed_two_wall_guide(cam, w, h, [p[0] for p in at(0.5)])[:4]
        acc = np.ones((h, w, 4), np.float32)
        a, hd = to_dev(torch, acc), hits_dev(torch, hit_records(*fields))
        o = torch.empty((h, w, 4), dtype=torch.float32, device="cuda")
        c = _lib.TemporalCamera(*[(C.c_float * 3)(*[float(x) for x in v]) for v in cam])
        torch.cuda.synchronize()
        mem, mb = torch.cuda.memory_allocated(), tp.get_int("models.bytes")
        assert _lib.lib().srt_temporal_accumulate(tp.handle, C.c_void_p(a.data_ptr()), 1, C.c_void_p(hd.data_ptr()), C.byref(c),
                                                  C.c_void_p(o.data_ptr())) == _lib.SRT_OK
        assert torch.cuda.memory_allocated() == mem and tp.get_int("models.bytes") == mb and tp.get_int("launches") == 2
        tp.synchronize()
        want = ref.accumulate(acc, 1, D.make_guide(*fields), cam)
        assert bits_equal(o.cpu().numpy(), want).all()
        with pytest.raises(S.SrtError) as e:
            bad = M.IDENTITY.copy()
            bad[7] = 0.5
            tp.set_models([M.IDENTITY, bad], [M.IDENTITY, M.IDENTITY])
        assert e.value.code == _lib.SRT_ERR_INVALID and tp.get_int("models") == 3


def test_enqueue_only_on_a_callers_stream(torch):
    """70x41, a caller's stream: two frames with the poses changed between them are enqueued back to back and read
    after one synchronise; the caller's pose array is overwritten with garbage as soon as each set_models returns."""
    from srt_amd import _lib
    from srt_amd.temporal import Temporal

    w, h = 70, 41
    lib = _lib.lib()
    frames = M.moving_two_wall_frames(w, h)[1:4]
    stream = torch.cuda.Stream()
    with Temporal(w, h, stream=stream) as tp:
        with torch.cuda.stream(stream):
            ins = [(to_dev(torch, a), hits_dev(torch, hit_records(*f))) for _, a, f, _ in frames]
            outs = [torch.empty((h, w, 4), dtype=torch.float32, device="cuda") for _ in ins]
            stream.synchronize()
            mem = None
            for (a, hd), o, (cam, _, _, poses) in zip(ins, outs, frames):
                arr = (_lib.TemporalModel * 2)()
                for k, (w2m, m2w) in enumerate(poses):
                    arr[k].world_to_model[:] = w2m.tolist()
                    arr[k].model_to_world[:] = m2w.tolist()
                assert lib.srt_temporal_set_models(tp.handle, arr, 2) == _lib.SRT_OK
                C.memset(arr, 0xFF, C.sizeof(arr))
                if mem is None:  # the first set_models allocated the poses' array; nothing does after it
                    mem = torch.cuda.memory_allocated()
                c = _lib.TemporalCamera(*[(C.c_float * 3)(*[float(x) for x in v]) for v in cam])
                assert lib.srt_temporal_accumulate(tp.handle, C.c_void_p(a.data_ptr()), 3, C.c_void_p(hd.data_ptr()),
                                                   C.byref(c), C.c_void_p(o.data_ptr())) == _lib.SRT_OK
                C.memset(C.byref(c), 0xFF, C.sizeof(c))
                assert tp.get_int("launches") == 2
            assert torch.cuda.memory_allocated() == mem
        stream.synchronize()
        got = [o.cpu().numpy() for o in outs]
        assert tp.get_int("frames") == 3
    ref = M.TemporalMotionRef(w, h)
    moved = []
    for g, (cam, acc, f, poses) in zip(got, frames):
        ref.set_models(poses)
        moved.append(ref.motion()[0].tolist())
        want = ref.accumulate(acc, 3, D.make_guide(*f), cam)
        assert bits_equal(g[..., :3], want[..., :3]).all() and (g[..., 3] == want[..., 3]).all()
    assert moved == [[False, False], [False, True], [False, True]]
    assert (want[..., 3] == 3).mean() > 0.2


# ---------------------------------------------------------------------------------------------------------------
# Rubik, end to end
# ---------------------------------------------------------------------------------------------------------------
RUBIK_W, RUBIK_H = 64, 48
SPIN_DEGREES = 2.0  # per frame, about the vertical axis through the centre of the cube's bounds
SPIN_FRAMES = 8
RUBIK_SHARE = 0.27  # of the hit pixels have N >= 4 at least: a third of the 0.810 the CPU gives


def spin_poses(scene):
    """Per frame k = 0..7 the pose of record 0 with the cube turned by (k + 1) * SPIN_DEGREES: model_to_world is the
    rotation about the vertical axis through the bounds' centre, `frame` its inverse (the inverse rotation)."""
    v = scene.verts["pos"].astype(np.float64)
    centre = (v.min(0) + v.max(0)) / 2
    poses = []
    for k in range(SPIN_FRAMES):
        rot = M.rotation("y", (k + 1) * SPIN_DEGREES)
        poses.append(M.pose_from_model(M.column_major(rot, centre - rot @ centre)))
    return poses


def posed_setup(setup, pose):
    """A copy of `setup` whose scene has record 0's frame replaced: what the oracle renders and traces."""
    s = copy.copy(setup)
    s.scene = copy.copy(setup.scene)
    s.scene.bvhs = setup.scene.bvhs.copy()
    s.scene.bvhs[0]["frame"] = pose[0]
    return s


def oracle_guide(setup):
    w, h = setup.width, setup.height
    o, d = D.camera_rays(*T.as_camera(setup.camera), w, h)
    rays = np.zeros(w * h, S.RAY_DTYPE)
    rays["o"], rays["d"], rays["t"] = o, d, np.float32(1e30)
    tri, t, nrm, _ = O.Oracle(setup.scene).trace_closest(setup.bvh_count, rays)
    return D.make_guide(tri.reshape(h, w), t.reshape(h, w), nrm.reshape(h, w, 3))


@pytest.fixture(scope="module")
def rubik_refs():
    """Oracle only: the hits of the pixel-centre rays under the 8 poses and the 256-spp frame of the last one."""
    setup = R.make_setup(RUBIK_W, RUBIK_H, show_model=True, models=[S.load_obj(OBJECTS / "Rubik" / "Rubik.obj")])
    poses = spin_poses(setup.scene)
    guides = [oracle_guide(posed_setup(setup, p)) for p in poses]
    ref_acc, _, _ = oracle_render(posed_setup(setup, poses[-1]), 256)
    return {"poses": poses, "guides": guides, "ref": D.mean_colour(ref_acc, 257)}


def test_end_to_end_on_rubik(torch, rubik_refs):
    """Eight frames of a still camera with the cube turning 2 degrees a frame, each a reset + 1 spp on the GPU after
    the frame went to the renderer, the query and the temporal object: the guide equals the oracle's hits on a scene
    with that frame, the temporal output equals the restatement fed with the read-back accumulation, the denoised
    output equals denoise_ref.atrous of it, and over the hit pixels with N >= 4 the temporal result is closer to the
    oracle's 256-spp frame of the last pose than the raw 1-spp mean.  On the CPU (the oracle's 1-spp frames +
    restatement) at 2 degrees: 814 of the 1005 hit pixels (81.0%) have N >= 4; MSE 0.155912 temporal against 2.812926
    raw (a history without poses, on the same pixels: 0.206141).  The asserted share is a third of the CPU's."""
    from srt_amd.denoise import Denoiser
    from srt_amd.query import Query
    from srt_amd.temporal import Temporal

    w, h = RUBIK_W, RUBIK_H
    setup = R.make_setup(w, h, show_model=True, models=[S.load_obj(OBJECTS / "Rubik" / "Rubik.obj")])
    dn_params = dict(passes=5, normal_squarings=5, sigma_color=3.0, sigma_depth=0.2)
    ref = M.TemporalMotionRef(w, h)
    cam = setup.camera
    rdr = R.Renderer(setup, device=0)
    try:
        with Temporal(w, h) as tp, Denoiser(w, h) as dn, Query(setup.scene) as q:
            q.set_bvh_count(setup.bvh_count)
            acc_ptr, _ = rdr.compute.image_pointers()
            for k, pose in enumerate(rubik_refs["poses"]):
                S.UpdateModelMatrix(rdr.compute, 0, pose[0])
                q.update_model_matrix(0, pose[0])
                set_both(tp, ref, [pose])
                rdr.render(1)  # the reset frame + one sample: accumFrames = 2
                rdr.finish()
                assert rdr.accum_frames == 2
                hits = q.closest(dn.primary_rays(cam))
                out = tp.accumulate(acc_ptr, 2, hits, cam)
                den = dn.run(out, 1, hits)
                dn.synchronize()
                assert tp.get_int("launches") == 2
                out, den, acc, hn = out.cpu().numpy(), den.cpu().numpy(), rdr.accum(), hits.numpy()
                g = rubik_refs["guides"][k]
                assert (hn["triangle"].reshape(h, w) == g["tri"]).all() and bits_equal(hn["t"].reshape(h, w), g["t"]).all()
                assert bits_equal(hn["normal"].reshape(h, w, 3), g["normal"]).all()
                want = ref.accumulate(acc, 2, g, cam)
                assert bits_equal(out[..., :3], want[..., :3]).all() and (out[..., 3] == want[..., 3]).all(), k
                assert bits_equal(den[..., :3], D.atrous(want[..., :3], g, **dn_params)).all(), k
    finally:
        rdr.close()
    hit = g["tri"] != D.MISS
    old = hit & (want[..., 3] >= 4)
    truth = rubik_refs["ref"]
    mse = lambda img: float(np.mean((img[old].astype(np.float64) - truth[old].astype(np.float64)) ** 2))  # noqa: E731
    raw = D.mean_colour(acc, 2)
    print(f"{int(old.sum())} of {int(hit.sum())} hit pixels have N >= 4 ({old.sum() / hit.sum():.3f}); "
          f"MSE temporal {mse(out[..., :3]):.6f}, raw 1-spp mean {mse(raw):.6f}")
    assert old.sum() >= RUBIK_SHARE * hit.sum()
    assert mse(out[..., :3]) < mse(raw)
