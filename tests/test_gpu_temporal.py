"""GPU: the temporal reprojection (include/srt_temporal.h, srt_amd.temporal.Temporal) against the independent
numpy float32 restatement of its definition (tests/temporal_ref.py, which never calls into the library): rgb bit
for bit (bits_equal treats any NaN as equal to any NaN) and N exactly, after every frame.

The Rubik references (oracle hits per camera, the oracle's 256-spp frame) are computed once per module and left
unchanged.
"""
import ctypes as C

import numpy as np
import pytest

import denoise_ref as D
import srt_amd as S
import temporal_ref as T
from srt_amd import render as R
from conftest import OBJECTS, bits_equal, oracle_render
from oracle import pyoracle as O

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (5, 1), (37, 23), (70, 41)]
# position, yaw, pitch: the first two are equal, then three small moves
CAMERAS = [((0, 0, 4), -90, 0), ((0, 0, 4), -90, 0), ((.15, .05, 3.9), -92, 1), ((.3, .1, 3.8), -94, 2),
           ((-.4, 0, 3.8), -84, -1)]
DEFAULTS = dict(max_history=32, depth_tol=0.05, normal_min=0.9)


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


def hit_records(tri, t, n, bvh):
    from srt_amd.query import HIT_DTYPE

    hits = np.zeros(tri.size, HIT_DTYPE)
    hits["triangle"], hits["t"], hits["normal"], hits["bvh"] = tri.reshape(-1), t.reshape(-1), n.reshape(-1, 3), bvh.reshape(-1)
    return hits


def two_wall_frames(w, h, cameras=CAMERAS, seed=7):
    """Per camera: (camera vectors, accumulation as a sum over 3 frames, guide fields (tri, t, normal, bvh))."""
    rng = np.random.default_rng(seed + 1000 * w + h)
    frames = []
    for pos, yaw, pitch in cameras:
        cam = T.camera_vectors(pos, yaw, pitch)
        accum = np.ones((h, w, 4), np.float32)
        accum[..., :3] = rng.uniform(0, 6, (h, w, 3)).astype(np.float32)
        frames.append((cam, accum, T.two_wall_guide(cam, w, h)))
    return frames


def to_dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def hits_dev(torch, hits):
    return torch.from_numpy(hits.view(np.int32).reshape(-1, 8).copy()).cuda()


def step(torch, tp, ref, cam, accum, fields, frames=3):
    """One frame through the GPU object and the restatement; asserts they agree and returns the restatement's."""
    got = tp.accumulate(to_dev(torch, accum), frames, hits_dev(torch, hit_records(*fields)), cam)
    tp.synchronize()
    got = got.cpu().numpy()
    want = ref.accumulate(accum, frames, D.make_guide(*fields), cam)
    bad = int((~bits_equal(got[..., :3], want[..., :3])).sum()), int((got[..., 3] != want[..., 3]).sum())
    print(f"frame {ref.frames - 1}: {bad[0]} colour components and {bad[1]} history lengths differ")
    assert bad == (0, 0)
    assert tp.get_int("launches") == 1
    return want


@pytest.mark.parametrize("w,h", SIZES)
def test_two_wall_scene_bit_exact(torch, w, h):
    """1x1, 5x1, 37x23 (no multiple of the 64 x 4 block) and 70x41 (several blocks in both directions): five cameras
    over a back wall and a nearer square in front of it, the GPU equal to the restatement after every frame.  On
    the restatement alone: frame 0 has no history, the repeated camera finds every hit pixel again, and the last
    move both reuses and rejects (the square's parallax uncovers wall that was hidden)."""
    from srt_amd.temporal import Temporal

    ref = T.TemporalRef(w, h)
    res, hit = [], []
    with Temporal(w, h) as tp:
        assert tp.params == pytest.approx(DEFAULTS)
        for cam, accum, fields in two_wall_frames(w, h):
            res.append(step(torch, tp, ref, cam, accum, fields))
            hit.append(fields[0] != D.MISS)
        assert tp.get_int("frames") == 5 and tp.get_int("history") == 1
    assert (res[0][..., 3] == 1).all()
    assert (res[1][..., 3][hit[1]] == 2).all() and (res[1][..., 3][~hit[1]] == 1).all()
    if w >= 37:
        n4 = res[4][..., 3][hit[4]]
        print(f"frame 4: {(n4 >= 2).mean():.3f} of hit pixels reuse, {(n4 == 1).mean():.3f} rejected, "
              f"{(~hit[4]).mean():.3f} miss, N up to {n4.max()}")
        assert (n4 >= 2).mean() >= 0.5 and (n4 == 1).mean() >= 0.02 and (~hit[4]).mean() >= 0.10
        assert (res[4][..., 3][~hit[4]] == 1).all()


def interior(mask):
    """Pixels whose 3 x 3 neighbourhood lies in `mask`: with the same camera twice a pixel reprojects onto itself up
    to rounding, so its taps are itself and, with a weight of a few ulps, one neighbour per axis."""
    m = mask.copy()
    for oy in (-1, 0, 1):
        for ox in (-1, 0, 1):
            m &= D._shift(mask, ox, oy, False)
    return m


REJECTIONS = ["bvh", "normal", "depth", "miss", "colour", "behind", "outside"]


@pytest.mark.parametrize("what", REJECTIONS)
def test_each_rejection_on_its_own(torch, what):
    """37x23, the first camera twice: with the unedited first frame every hit pixel has N == 2 on the second.  One
    property of the FIRST frame is then edited by hand in a block of back-wall pixels (or its camera turned) and
    the block's interior falls back to N == 1; GPU and restatement agree on both frames either way."""
    from srt_amd.temporal import Temporal

    w, h = 37, 23
    (cam0, acc0, f0), (cam1, acc1, f1) = two_wall_frames(w, h)[:2]
    base = T.TemporalRef(w, h)
    base.accumulate(acc0, 3, D.make_guide(*f0), cam0)
    n_base = base.accumulate(acc1, 3, D.make_guide(*f1), cam1)[..., 3]
    hit = f1[0] != D.MISS
    assert (n_base[hit] == 2).all()

    tri, t, nrm, bvh = (a.copy() for a in f0)
    acc0 = acc0.copy()
    block = np.zeros((h, w), bool)
    block[7:15, 8:17] = True
    block &= (f0[3] == 0) & (f0[0] != D.MISS)  # back-wall pixels only
    where = interior(block)
    assert where.sum() >= 6
    if what == "bvh":
        bvh[block] = 5
    elif what == "normal":
        nrm[block] = (0, 0, -1)
    elif what == "depth":
        t[block] = t[block] * np.float32(1.2)  # |a - 1.2a| = 0.2a against 0.05 * 2.2a
    elif what == "miss":
        tri[block] = D.MISS
    elif what == "colour":
        acc0[block, 1] = np.inf
    elif what == "behind":  # the previous camera looked the other way: a <= 0 for every point
        cam0 = T.camera_vectors(CAMERAS[0][0], 90, 0)
        a, _, _ = T.reproject(f1[1], cam1, cam0, w, h)
        assert (a[hit] <= 0).all()
        where = hit
    elif what == "outside":  # the previous camera was turned by 60 degrees: in front of it, but off its image
        cam0 = T.camera_vectors(CAMERAS[0][0], -30, 0)
        a, uu, vv = T.reproject(f1[1], cam1, cam0, w, h)
        assert (a[hit] > 0).all() and ((uu[hit] < -1) | (uu[hit] >= w)).all()
        where = hit
    ref = T.TemporalRef(w, h)
    with Temporal(w, h) as tp:
        step(torch, tp, ref, cam0, acc0, (tri, t, nrm, bvh))
        n = step(torch, tp, ref, cam1, acc1, f1)[..., 3]
    assert (n[where] == 1).all() and (n[where] != n_base[where]).all()
    if what not in ("behind", "outside"):
        assert (n[hit & interior(~block)] == 2).all()  # away from the block nothing changes


def test_nonfinite_current_colours(torch):
    """A NaN (or Inf) sample over a pixel with history is replaced by the history and N is not incremented; without
    history it passes through.  With one camera throughout a pixel reprojects onto itself up to rounding, so besides
    itself it may take one neighbour per axis with a weight of a few ulps (below 1e-4): the history of q and r is
    their own previous value to that accuracy, and pixels next to p, q and r are left out of the counts."""
    from srt_amd.temporal import Temporal

    w, h = 37, 23
    frames = two_wall_frames(w, h, CAMERAS[:1] * 3)
    hit = frames[0][2][0] != D.MISS
    ys, xs = np.nonzero(interior(hit))
    p, q, r = [(ys[k], xs[k]) for k in (0, len(ys) // 2, len(ys) - 1)]
    frames[0][1][p][:3] = (np.nan, 1.0, 2.0)  # no history yet
    frames[1][1][q][0] = np.nan               # history of one frame
    frames[1][1][r][2] = np.inf
    ref = T.TemporalRef(w, h)
    with Temporal(w, h) as tp:
        r0, r1, r2 = (step(torch, tp, ref, cam, accum, fields) for cam, accum, fields in frames)
    assert np.isnan(r0[p][0]) and r0[p][3] == 1
    assert np.isfinite(r1[p][:3]).all() and r1[p][3] in (1, 2)  # the NaN history itself was not reused
    for s in (q, r):
        assert r1[s][3] == 1 and np.allclose(r1[s][:3], r0[s][:3], rtol=0, atol=1e-4)  # the history, not counted
        assert r2[s][3] == 2
    others = interior(hit).copy()
    for s in (p, q, r):
        others[s[0] - 1:s[0] + 2, s[1] - 1:s[1] + 2] = False
    assert (r1[..., 3][others] == 2).all() and (r2[..., 3][others] == 3).all()
    assert np.isfinite(r2[..., :3]).all()


def test_max_history(torch):
    """max_history = 3: eight frames of one camera leave N == 3 on hit pixels.  max_history = 1: N' = 1, so the output
    is hist + 1.0f * (C - hist): C up to the two roundings of that expression (at most 2^-23 * (|C| + |hist|) each,
    colours below 2 here: 1e-6 in all), and bit-identical to the restatement."""
    from srt_amd.temporal import Temporal

    w, h = 37, 23
    frames = two_wall_frames(w, h, CAMERAS[:1] * 8)
    hit = frames[0][2][0] != D.MISS
    ref = T.TemporalRef(w, h, max_history=3)
    with Temporal(w, h) as tp:
        tp.set_params(max_history=3)
        assert tp.get_int("max_history") == 3
        for cam, accum, fields in frames:
            out = step(torch, tp, ref, cam, accum, fields)
        assert tp.get_int("frames") == 8
    assert (out[..., 3][hit] == 3).all() and (out[..., 3][~hit] == 1).all()
    ref = T.TemporalRef(w, h, max_history=1)
    with Temporal(w, h) as tp:
        tp.set_params(max_history=1)
        for cam, accum, fields in frames[:3]:
            out = step(torch, tp, ref, cam, accum, fields)
            assert (out[..., 3] == 1).all()
            assert np.abs(out[..., :3] - D.mean_colour(accum, 3)).max() <= 1e-6
            assert bits_equal(out[..., :3][~hit], D.mean_colour(accum, 3)[~hit]).all()


def test_reset(torch):
    from srt_amd.temporal import Temporal

    w, h = 37, 23
    frames = two_wall_frames(w, h, CAMERAS[:1] * 4)
    hit = frames[0][2][0] != D.MISS
    ref = T.TemporalRef(w, h)
    with Temporal(w, h) as tp:
        assert tp.get_int("history") == 0 and tp.get_int("frames") == 0
        step(torch, tp, ref, *frames[0])
        assert tp.get_int("history") == 1 and tp.get_int("frames") == 1
        out = step(torch, tp, ref, *frames[1])
        assert (out[..., 3][hit] == 2).all() and tp.get_int("frames") == 2
        tp.reset()
        ref.reset()
        assert tp.get_int("history") == 0 and tp.get_int("frames") == 0
        out = step(torch, tp, ref, *frames[2])
        assert (out[..., 3] == 1).all() and bits_equal(out[..., :3], D.mean_colour(frames[2][1], 3)).all()
        assert tp.get_int("history") == 1 and tp.get_int("frames") == 1
        out = step(torch, tp, ref, *frames[3])
        assert (out[..., 3][hit] == 2).all()


def test_parameter_rejection(torch):
    """Out-of-range values return SRT_ERR_INVALID and leave the state unchanged; so do bad arguments of accumulate."""
    from srt_amd import _lib
    from srt_amd.temporal import Temporal

    w, h = 37, 23
    cam, accum, fields = two_wall_frames(w, h)[0]
    with Temporal(w, h) as tp:
        tp.set_params(max_history=7, depth_tol=0.1, normal_min=0.5)
        want = dict(max_history=7, depth_tol=0.1, normal_min=0.5)
        for bad in (dict(max_history=0), dict(max_history=65536), dict(depth_tol=0.0), dict(depth_tol=float("nan")),
                    dict(normal_min=1.5), dict(depth_tol=float("inf")), dict(normal_min=-1.5)):
            with pytest.raises(S.SrtError) as e:
                tp.set_params(**bad)
            assert e.value.code == 1
            assert tp.params == pytest.approx(want) and tp.get_int("max_history") == 7
        tp.set_params(max_history=65535, depth_tol=1e-30, normal_min=-1.0)
        v = C.c_int()
        assert _lib.lib().srt_temporal_get_int(tp.handle, b"no.such.name", C.byref(v)) == _lib.SRT_ERR_NOT_FOUND
        a, hd = to_dev(torch, accum), hits_dev(torch, hit_records(*fields))
        o = torch.empty((h, w, 4), dtype=torch.float32, device="cuda")
        acc = _lib.lib().srt_temporal_accumulate
        P = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
        c = _lib.TemporalCamera()
        inv = _lib.SRT_ERR_INVALID
        assert acc(tp.handle, P(a), 0, P(hd), C.byref(c), P(o)) == inv      # frames < 1
        assert acc(tp.handle, None, 1, P(hd), C.byref(c), P(o)) == inv
        assert acc(tp.handle, P(a), 1, None, C.byref(c), P(o)) == inv
        assert acc(tp.handle, P(a), 1, P(hd), None, P(o)) == inv
        assert acc(tp.handle, P(a), 1, P(hd), C.byref(c), None) == inv
        assert acc(tp.handle, P(a), 1, P(hd), C.byref(c), P(a)) == inv      # out aliases accum
        assert acc(tp.handle, C.c_void_p(a.data_ptr() + 4), 1, P(hd), C.byref(c), P(o)) == inv  # misaligned
        assert tp.get_int("frames") == 0 and tp.get_int("history") == 0 and tp.get_int("launches") == 0


def test_enqueue_only_on_a_callers_stream(torch):
    """Two frames enqueued back to back on a caller's stream and read after one synchronise equal the restatement;
    accumulate allocates nothing and is one launch."""
    from srt_amd import _lib
    from srt_amd.temporal import Temporal

    w, h = 70, 41
    (cam0, acc0, f0), _, (cam2, acc2, f2) = two_wall_frames(w, h)[:3]
    stream = torch.cuda.Stream()
    with Temporal(w, h, stream=stream) as tp:
        assert tp.get_int("scratch.bytes") == 72 * w * h and tp.get_int("width") == w and tp.get_int("height") == h
        assert int(_lib.lib().srt_temporal_stream(tp.handle)) == stream.cuda_stream
        with torch.cuda.stream(stream):
            ins = [(to_dev(torch, a), hits_dev(torch, hit_records(*f))) for a, f in ((acc0, f0), (acc2, f2))]
            outs = [torch.empty((h, w, 4), dtype=torch.float32, device="cuda") for _ in ins]
            stream.synchronize()
            scratch, mem = tp.get_int("scratch.bytes"), torch.cuda.memory_allocated()
            for (a, hd), o, cam in zip(ins, outs, (cam0, cam2)):
                c = _lib.TemporalCamera(*[(C.c_float * 3)(*[float(x) for x in v]) for v in cam])
                assert _lib.lib().srt_temporal_accumulate(tp.handle, C.c_void_p(a.data_ptr()), 3, C.c_void_p(hd.data_ptr()),
                                                          C.byref(c), C.c_void_p(o.data_ptr())) == _lib.SRT_OK
                assert tp.get_int("launches") == 1
            assert torch.cuda.memory_allocated() == mem and tp.get_int("scratch.bytes") == scratch
        stream.synchronize()
        got = [o.cpu().numpy() for o in outs]
        assert tp.get_int("frames") == 2
    ref = T.TemporalRef(w, h)
    for g, (cam, acc, f) in zip(got, ((cam0, acc0, f0), (cam2, acc2, f2))):
        want = ref.accumulate(acc, 3, D.make_guide(*f), cam)
        assert bits_equal(g[..., :3], want[..., :3]).all() and (g[..., 3] == want[..., 3]).all()
    assert (want[..., 3] == 2).mean() > 0.2


# ---------------------------------------------------------------------------------------------------------------
# Rubik, end to end
# ---------------------------------------------------------------------------------------------------------------
RUBIK_W, RUBIK_H = 64, 48
# per frame after the first: MoveRight(delta), Rotate(yaw offset in degrees, 0): the camera circles the cube a little
RUBIK_PATH = [(0.5, -1.0)] * 7


def rubik_cameras(setup):
    """Moves setup.camera along RUBIK_PATH, yielding after each position (8 in all)."""
    yield setup.camera
    for delta, yaw in RUBIK_PATH:
        setup.camera.MoveRight(delta)
        setup.camera.Rotate(yaw, 0.0)
        yield setup.camera


def oracle_guide(setup):
    w, h = setup.width, setup.height
    o, d = D.camera_rays(*T.as_camera(setup.camera), w, h)
    rays = np.zeros(w * h, S.RAY_DTYPE)
    rays["o"], rays["d"], rays["t"] = o, d, np.float32(1e30)
    tri, t, nrm, _ = O.Oracle(setup.scene).trace_closest(setup.bvh_count, rays)
    return D.make_guide(tri.reshape(h, w), t.reshape(h, w), nrm.reshape(h, w, 3))


@pytest.fixture(scope="module")
def rubik_refs():
    """Oracle only: the hits of the pixel-centre rays of the 8 cameras and the 256-spp frame of the last one."""
    setup = R.make_setup(RUBIK_W, RUBIK_H, show_model=True, models=[S.load_obj(OBJECTS / "Rubik" / "Rubik.obj")])
    guides = [oracle_guide(setup) for _ in rubik_cameras(setup)]
    ref_acc, _, _ = oracle_render(setup, 256)
    return {"guides": guides, "ref": D.mean_colour(ref_acc, 257)}


def test_end_to_end_on_rubik(torch, rubik_refs):
    """Eight frames along a small camera path, each a reset + 1 spp on the GPU with its guide traced on the GPU,
    accumulated on the context's own device image and then denoised: the temporal output equals the restatement
    fed with the read-back accumulation and the oracle's hits, the denoised output equals denoise_ref.atrous of it,
    and over the hit pixels with N >= 4 the temporal result is closer to the oracle's 256-spp frame of the last
    camera than the raw 1-spp mean.  On the CPU (the oracle's 1-spp frames + restatement): 1030 of the 1041 hit
    pixels (98.9%) have N >= 4; MSE 0.087878 temporal against 0.397169 raw."""
    from srt_amd.denoise import Denoiser
    from srt_amd.query import Query
    from srt_amd.temporal import Temporal

    w, h = RUBIK_W, RUBIK_H
    setup = R.make_setup(w, h, show_model=True, models=[S.load_obj(OBJECTS / "Rubik" / "Rubik.obj")])
    dn_params = dict(passes=5, normal_squarings=5, sigma_color=3.0, sigma_depth=0.2)
    ref = T.TemporalRef(w, h)
    rdr = R.Renderer(setup, device=0)
    try:
        with Temporal(w, h) as tp, Denoiser(w, h) as dn, Query(setup.scene) as q:
            q.set_bvh_count(setup.bvh_count)
            acc_ptr, _ = rdr.compute.image_pointers()
            for k, cam in enumerate(rubik_cameras(setup)):
                c = rdr.compute
                c.SetVec3("cameraOrigin", cam.getOrigin())
                c.SetVec3("cameraDirection", cam.getForward())
                c.SetVec3("cameraUp", cam.getUpVector())
                c.SetVec3("cameraRight", cam.getRightVector())
                rdr.render(1)  # the reset frame + one sample: accumFrames = 2
                rdr.finish()
                assert rdr.accum_frames == 2
                hits = q.closest(dn.primary_rays(cam))
                out = tp.accumulate(acc_ptr, 2, hits, cam)
                den = dn.run(out, 1, hits)
                dn.synchronize()
                out, den, acc, hn = out.cpu().numpy(), den.cpu().numpy(), rdr.accum(), hits.numpy()
                g = rubik_refs["guides"][k]
                assert (hn["triangle"].reshape(h, w) == g["tri"]).all() and bits_equal(hn["t"].reshape(h, w), g["t"]).all()
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
    assert old.sum() >= 0.30 * hit.sum()
    assert mse(out[..., :3]) < mse(raw)
