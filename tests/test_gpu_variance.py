"""GPU: the temporal luminance moments and the variance-guided filter (include/srt_variance.h) against the
independent numpy float32 restatement (tests/variance_ref.py, which never calls into the library), bit for bit
(bits_equal treats any NaN as equal to any NaN) after every frame.

The Rubik references (tests/variance_scenes.py: the oracle's hits per camera and its 256-spp frame of the last one)
are computed once per process and left unchanged.
"""
import ctypes as C
import gc

import numpy as np
import pytest

import denoise_ref as D
import srt_amd as S
import temporal_motion_ref as M
import variance_ref as V
import variance_scenes as VS
from conftest import bits_equal

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (5, 1), (37, 23), (70, 41)]
MIN_HISTORY = 4


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


def same(got, want):
    return bool(bits_equal(np.asarray(got), np.asarray(want)).all())


def run_sequence(torch, w, h, frames, with_poses, passes):
    """Every frame through a Temporal with moments, a second plain Temporal, a Denoiser with variance and the
    restatement; asserts equality after every frame and returns the restatement's last (out, moments, C, var, guide)."""
    from srt_amd.denoise import Denoiser
    from srt_amd.temporal import Temporal

    ref = V.VarianceTemporalRef(w, h)
    with Temporal(w, h) as tp, Temporal(w, h) as plain, Denoiser(w, h) as dn:
        tp.enable_moments()
        dn.enable_variance()
        dn.set_params(passes=passes)
        for k, (cam, accum, fields, poses) in enumerate(frames):
            if with_poses:
                for t in (tp, plain):
                    t.set_models([p[0] for p in poses], [p[1] for p in poses])
                ref.set_models(poses)
            a, hd = to_dev(torch, accum), hits_dev(torch, hit_records(*fields))
            out, mom = tp.accumulate_moments(a, 3, hd, cam)
            out_plain = plain.accumulate(a, 3, hd, cam)
            den, var = dn.run_variance(out, 1, hd, mom)
            dn.synchronize()
            plain.synchronize()
            g = D.make_guide(*fields)
            want_out, want_mom = ref.accumulate_moments(accum, 3, g, cam)
            want_c, want_var = V.run_variance(want_out, 1, g, want_mom, passes=passes)
            got = [x.cpu().numpy() for x in (out, out_plain, mom, den, var)]
            bad = [int((~bits_equal(x, y)).sum()) for x, y in ((got[0], want_out), (got[1], want_out), (got[2], want_mom),
                                                               (got[3][..., :3], want_c), (got[4], want_var))]
            print(f"frame {k}: differing out {bad[0]}, plain out {bad[1]}, moments {bad[2]}, filtered {bad[3]}, variance {bad[4]}")
            assert bad == [0, 0, 0, 0, 0], k
            assert (got[3][..., 3] == 1).all()
            assert tp.get_int("launches") == plain.get_int("launches") and dn.get_int("launches") == 1 + passes
    return want_out, want_mom, want_c, want_var, g


@pytest.mark.parametrize("passes", [1, 5])
@pytest.mark.parametrize("with_poses", [True, False], ids=["motion", "static"])
@pytest.mark.parametrize("w,h", SIZES)
def test_two_wall_scene_bit_exact(torch, w, h, with_poses, passes):
    """1x1, 5x1, 37x23 and 70x41, five frames of the moving two-wall scene with poses (the motion instance) and without
    (the static one), 1 and 5 passes: `out` equal to the restatement and to a plain accumulate on a second object, the
    moments, the variance-filtered colour and the variance equal to the restatement, after every frame.  On the
    restatement alone (tests/test_variance_api.py prints the same on the CPU): from 37 wide the last frame has at least
    2% of its hit pixels with N < 4 (the spatial branch) and at least 50% with N >= 4, and at least 10% of the image is
    a miss -- at 37x23 0.120 / 0.880 / 0.589 with poses and 0.197 / 0.803 / 0.589 without."""
    out, mom, c, var, g = run_sequence(torch, w, h, M.moving_two_wall_frames(w, h), with_poses, passes)
    if w >= 37:
        hit = g["tri"] != D.MISS
        n = mom[..., 3][hit]
        assert (n < MIN_HISTORY).mean() >= 0.02 and (n >= MIN_HISTORY).mean() >= 0.50 and (~hit).mean() >= 0.10
        assert (var[~hit] == 0).all() and (var[hit] > 0).mean() > 0.9 and not same(c, out[..., :3])


def test_nonfinite_input(torch):
    """37x23, a NaN and an Inf put into `accum` at two interior pixels of the back wall in frames 0 and 3: the GPU
    equals the restatement on every frame (run_sequence asserts it), the repaired pixels and the poisoned ones are
    where the restatement puts them, and no pixel that was finite going into the filter comes out non-finite."""
    w, h = 37, 23
    frames = M.moving_two_wall_frames(w, h)
    wall = M.interior((frames[0][2][0] != D.MISS) & (frames[0][2][3] == 0) & (frames[3][2][0] != D.MISS) & (frames[3][2][3] == 0))
    ys, xs = np.nonzero(wall)
    assert len(ys) >= 2
    p, q = (ys[0], xs[0]), (ys[-1], xs[-1])
    for k in (0, 3):  # frame 0 has no history to repair from: the filter itself meets the NaN and the Inf
        frames[k][1][p][0] = np.nan
        frames[k][1][q][1] = np.inf
    for passes in (1, 5):
        out, mom, c, var, g = run_sequence(torch, w, h, frames, True, passes)
        fin_in = np.isfinite(out[..., :3]).all(-1)
        assert np.isfinite(c[fin_in]).all() and np.isfinite(var[fin_in]).all()
    # frame 0 on the restatement (the GPU equalled it above): both samples reach the filter as they are, their
    # moments non-finite too, and every pixel that went in finite comes out finite, colour and variance
    ref = V.VarianceTemporalRef(w, h)
    cam, accum, fields, poses = frames[0]
    ref.set_models(poses)
    o, m = ref.accumulate_moments(accum, 3, D.make_guide(*fields), cam)
    bad = ~np.isfinite(o[..., :3]).all(-1)
    assert bad.sum() == 2 and bad[p] and bad[q] and not np.isfinite(m[p][:2]).any() and not np.isfinite(m[q][:2]).any()
    for passes in (1, 5):
        cf, vf = V.run_variance(o, 1, D.make_guide(*fields), m, passes=passes)
        assert np.isfinite(cf[~bad]).all() and np.isfinite(vf[~bad]).all()


def test_lifecycle_and_no_allocation(torch):
    """run_variance before enable_variance and accumulate_moments before enable_moments give SRT_ERR_INVALID, as do
    passes == 0 and a misaligned or missing moments pointer; the enables are idempotent and report 16 and 8 B a pixel
    while scratch.bytes stays; neither accumulate_moments nor run_variance allocates (raw ctypes calls with every
    buffer made beforehand); launches == 1 + passes."""
    from srt_amd import _lib
    from srt_amd.denoise import Denoiser
    from srt_amd.temporal import Temporal

    w, h = 37, 23
    lib, inv = _lib.lib(), _lib.SRT_ERR_INVALID
    cam, accum, fields, _ = M.moving_two_wall_frames(w, h)[0]
    a, hd = to_dev(torch, accum), hits_dev(torch, hit_records(*fields))
    o, m, den = (torch.empty((h, w, 4), dtype=torch.float32, device="cuda") for _ in range(3))
    var = torch.empty((h, w), dtype=torch.float32, device="cuda")
    c = _lib.TemporalCamera(*[(C.c_float * 3)(*[float(x) for x in v]) for v in cam])
    P = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    with Temporal(w, h) as tp, Denoiser(w, h) as dn:
        assert tp.get_int("moments.bytes") == 0 and dn.get_int("variance.bytes") == 0
        assert lib.srt_temporal_accumulate_moments(tp.handle, P(a), 3, P(hd), C.byref(c), P(o), P(m)) == inv
        assert lib.srt_denoise_run_variance(dn.handle, P(a), 3, P(hd), P(m), P(den), None, P(var)) == inv
        with pytest.raises(S.SrtError) as e:
            dn.run_variance(a, 3, hd, m)
        assert e.value.code == inv and tp.get_int("frames") == 0
        for _ in range(2):
            tp.enable_moments()
            dn.enable_variance()
            assert tp.get_int("moments.bytes") == 16 * w * h and dn.get_int("variance.bytes") == 8 * w * h
            assert tp.get_int("scratch.bytes") == 72 * w * h and dn.get_int("scratch.bytes") == 48 * w * h
        assert lib.srt_temporal_accumulate_moments(tp.handle, P(a), 3, P(hd), C.byref(c), P(o), None) == inv
        assert lib.srt_temporal_accumulate_moments(tp.handle, P(a), 3, P(hd), C.byref(c), P(o), C.c_void_p(m.data_ptr() + 8)) == inv
        assert lib.srt_denoise_run_variance(dn.handle, P(o), 1, P(hd), None, P(den), None, None) == inv
        assert lib.srt_denoise_run_variance(dn.handle, P(o), 1, P(hd), C.c_void_p(m.data_ptr() + 4), P(den), None, None) == inv
        assert lib.srt_denoise_run_variance(dn.handle, P(o), 1, P(hd), P(m), None, None, P(var)) == inv
        dn.set_params(passes=0)
        assert lib.srt_denoise_run_variance(dn.handle, P(o), 1, P(hd), P(m), P(den), None, P(var)) == inv
        assert "passes" in _lib.last_error() and tp.get_int("frames") == 0
        with pytest.raises(S.SrtError):
            dn.set_variance_params(sigma_lum=0.0)
        with pytest.raises(S.SrtError):
            dn.set_variance_params(min_history=0)
        assert dn.variance_params == {"sigma_lum": 1.0, "min_history": 4}
        ref = V.VarianceTemporalRef(w, h)
        want_out, want_mom = ref.accumulate_moments(accum, 3, D.make_guide(*fields), cam)
        for passes in (3, 1):
            dn.set_params(passes=passes)
            out8 = torch.empty((h, w, 4), dtype=torch.uint8, device="cuda")
            tp.reset()
            torch.cuda.synchronize()
            mem = torch.cuda.memory_allocated()
            assert lib.srt_temporal_accumulate_moments(tp.handle, P(a), 3, P(hd), C.byref(c), P(o), P(m)) == _lib.SRT_OK
            tp.synchronize()
            assert lib.srt_denoise_run_variance(dn.handle, P(o), 1, P(hd), P(m), P(den), P(out8), P(var)) == _lib.SRT_OK
            assert torch.cuda.memory_allocated() == mem
            assert dn.get_int("launches") == 1 + passes and tp.get_int("launches") == 1
            dn.synchronize()
            want_c, want_var = V.run_variance(want_out, 1, D.make_guide(*fields), want_mom, passes=passes)
            assert same(o.cpu().numpy(), want_out) and same(m.cpu().numpy(), want_mom)
            assert same(den.cpu().numpy()[..., :3], want_c) and same(var.cpu().numpy(), want_var)
            # the sRGB8 output alone, no variance output: the same colours through the context's encoding
            den.zero_()
            only8 = torch.empty_like(out8)
            assert lib.srt_denoise_run_variance(dn.handle, P(o), 1, P(hd), P(m), None, P(only8), None) == _lib.SRT_OK
            dn.synchronize()
            assert (only8 == out8).all() and (only8[..., 3] == 255).all() and (den == 0).all()
        dn.set_variance_params(sigma_lum=2.5, min_history=2)
        got_c, got_var = dn.run_variance(o, 1, hd, m)
        dn.synchronize()
        want_c, want_var = V.run_variance(want_out, 1, D.make_guide(*fields), want_mom, passes=1, sigma_lum=2.5, min_history=2)
        assert same(got_c.cpu().numpy()[..., :3], want_c) and same(got_var.cpu().numpy(), want_var)


def test_mixed_calls_and_reset(torch):
    """37x23: moments, moments, plain, moments, moments, reset, moments -- the frame after the plain call and the one
    after the reset carry (L, L*L, 1) while the colour follows its own history; equal to the restatement throughout."""
    from srt_amd.temporal import Temporal

    w, h = 37, 23
    frames = M.moving_two_wall_frames(w, h)
    ref = V.VarianceTemporalRef(w, h)
    with Temporal(w, h) as tp:
        tp.enable_moments()
        for k, (cam, accum, fields, poses) in enumerate(frames + frames[:1]):
            if k == 5:
                tp.reset()
                ref.reset()
            tp.set_models([p[0] for p in poses], [p[1] for p in poses])
            ref.set_models(poses)
            a, hd, g = to_dev(torch, accum), hits_dev(torch, hit_records(*fields)), D.make_guide(*fields)
            if k == 2:
                got = tp.accumulate(a, 3, hd, cam)
                tp.synchronize()
                assert same(got.cpu().numpy(), ref.accumulate(accum, 3, g, cam))
                continue
            out, mom = tp.accumulate_moments(a, 3, hd, cam)
            tp.synchronize()
            want_out, want_mom = ref.accumulate_moments(accum, 3, g, cam)
            assert same(out.cpu().numpy(), want_out) and same(mom.cpu().numpy(), want_mom), k
            if k in (0, 3, 5):
                assert (want_mom[..., 3] == 1).all()
            if k == 3:
                assert (want_out[..., 3] >= 2).mean() > 0.2
        assert tp.get_int("frames") == 1


def test_unchanged_behaviour_with_both_enabled(torch):
    """70x41: on objects with moments and variance enabled (and used in between), srt_temporal_accumulate and
    srt_denoise_run give the bits a fresh pair of objects gives, on every frame."""
    from srt_amd.denoise import Denoiser
    from srt_amd.temporal import Temporal

    w, h = 70, 41
    with Temporal(w, h) as tp, Temporal(w, h) as fresh_tp, Denoiser(w, h) as dn, Denoiser(w, h) as fresh_dn:
        tp.enable_moments()
        dn.enable_variance()
        for k, (cam, accum, fields, poses) in enumerate(M.moving_two_wall_frames(w, h)):
            a, hd = to_dev(torch, accum), hits_dev(torch, hit_records(*fields))
            for t in (tp, fresh_tp):
                t.set_models([p[0] for p in poses], [p[1] for p in poses])
            if k == 1:  # the variance path runs on the same objects in between
                out, mom = tp.accumulate_moments(a, 3, hd, cam)
                dn.run_variance(out, 1, hd, mom)
            else:
                out = tp.accumulate(a, 3, hd, cam)
            want = fresh_tp.accumulate(a, 3, hd, cam)
            den, den8 = dn.run(out, 1, hd, srgb=True)
            want_den, want_den8 = fresh_dn.run(want, 1, hd, srgb=True)
            torch.cuda.synchronize()
            assert same(out.cpu().numpy(), want.cpu().numpy()) and same(den.cpu().numpy(), want_den.cpu().numpy()), k
            assert (den8 == want_den8).all()
            assert dn.get_int("launches") == 5 and tp.get_int("launches") == 2


def test_enqueue_only_on_a_callers_stream(torch):
    """70x41, a caller's stream: three frames of accumulate_moments + run_variance are enqueued back to back by raw
    calls, allocate nothing, and are read after one synchronise."""
    from srt_amd import _lib
    from srt_amd.denoise import Denoiser
    from srt_amd.temporal import Temporal

    w, h = 70, 41
    lib = _lib.lib()
    frames = M.moving_two_wall_frames(w, h)[1:4]
    stream = torch.cuda.Stream()
    P = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    with Temporal(w, h, stream=stream) as tp, Denoiser(w, h, stream=stream) as dn:
        tp.enable_moments()
        dn.enable_variance()
        with torch.cuda.stream(stream):
            ins = [(to_dev(torch, a), hits_dev(torch, hit_records(*f))) for _, a, f, _ in frames]
            bufs = [[torch.empty((h, w, 4), dtype=torch.float32, device="cuda") for _ in range(3)]
                    + [torch.empty((h, w), dtype=torch.float32, device="cuda")] for _ in ins]
            stream.synchronize()
            # Tensors of earlier tests can still sit in garbage cycles (a pytest.raises traceback holds the frames of the
            # failed call); collected in the loop below they would lower the count, whenever the collector happens to run.
            gc.collect()
            mem = torch.cuda.memory_allocated()
            for (a, hd), (o, m, d, v), (cam, _, _, _) in zip(ins, bufs, frames):
                c = _lib.TemporalCamera(*[(C.c_float * 3)(*[float(x) for x in vec]) for vec in cam])
                assert lib.srt_temporal_accumulate_moments(tp.handle, P(a), 3, P(hd), C.byref(c), P(o), P(m)) == _lib.SRT_OK
                C.memset(C.byref(c), 0xFF, C.sizeof(c))
                assert lib.srt_denoise_run_variance(dn.handle, P(o), 1, P(hd), P(m), P(d), None, P(v)) == _lib.SRT_OK
            assert torch.cuda.memory_allocated() == mem
        stream.synchronize()
        got = [[t.cpu().numpy() for t in b] for b in bufs]
    ref = V.VarianceTemporalRef(w, h)
    for (o, m, d, v), (cam, acc, f, _) in zip(got, frames):
        g = D.make_guide(*f)
        want_out, want_mom = ref.accumulate_moments(acc, 3, g, cam)
        want_c, want_var = V.run_variance(want_out, 1, g, want_mom)
        assert same(o, want_out) and same(m, want_mom) and same(d[..., :3], want_c) and same(v, want_var)
    assert (want_mom[..., 3] == 3).mean() > 0.2


# ---------------------------------------------------------------------------------------------------------------
# Rubik, end to end
# ---------------------------------------------------------------------------------------------------------------
QUALITY_PASSES = 2


def test_end_to_end_on_rubik(torch):
    """Rubik 64x48, the 8 orbit frames, each a reset + 1 spp on the GPU: renderer -> query -> accumulate_moments ->
    run_variance.  The accumulation equals the oracle's, the guide the oracle's hits, the temporal output and the
    moments the restatement's, the variance-filtered colour and variance the restatement's, at the default 5 passes and
    at 2.  On the GPU's last frame, over the hit pixels and after x/(1+x), the 2-pass variance-guided result is strictly
    closer to the oracle's 256-spp frame than the temporal output it was fed: on the CPU (tests/test_variance_api.py,
    the same bits) 0.006213 against 0.007654.  At 5 passes it is not (0.008880: the steps 4-16 span much of the cube at
    this size), which DESIGN.md section 5 records."""
    from srt_amd import render as R
    from srt_amd.denoise import Denoiser
    from srt_amd.query import Query
    from srt_amd.temporal import Temporal

    w, h = VS.RUBIK_W, VS.RUBIK_H
    seq = VS.orbit()
    setup = VS.rubik_setup()
    ref = V.VarianceTemporalRef(w, h)
    rdr = R.Renderer(setup, device=0)
    try:
        with Temporal(w, h) as tp, Denoiser(w, h) as dn, Denoiser(w, h) as dn2, Query(setup.scene) as q:
            tp.enable_moments()
            dn.enable_variance()
            dn2.enable_variance()
            dn2.set_params(passes=QUALITY_PASSES)
            q.set_bvh_count(setup.bvh_count)
            acc_ptr, _ = rdr.compute.image_pointers()
            for k, cam in enumerate(VS.orbit_cameras(setup)):
                c = rdr.compute
                c.SetVec3("cameraOrigin", cam.getOrigin())
                c.SetVec3("cameraDirection", cam.getForward())
                c.SetVec3("cameraUp", cam.getUpVector())
                c.SetVec3("cameraRight", cam.getRightVector())
                rdr.render(1)  # the reset frame + one sample: accumFrames = 2
                rdr.finish()
                hits = q.closest(dn.primary_rays(cam))
                out, mom = tp.accumulate_moments(acc_ptr, 2, hits, cam)
                den, var = dn.run_variance(out, 1, hits, mom)
                den2, var2 = dn2.run_variance(out, 1, hits, mom)
                torch.cuda.synchronize()
                acc, hn = rdr.accum(), hits.numpy()
                g = seq["guides"][k]
                assert same(acc, seq["accs"][k]), k
                assert (hn["triangle"].reshape(h, w) == g["tri"]).all() and same(hn["t"].reshape(h, w), g["t"])
                assert same(hn["normal"].reshape(h, w, 3), g["normal"])
                want_out, want_mom = ref.accumulate_moments(acc, 2, g, seq["cams"][k])
                assert same(out.cpu().numpy(), want_out) and same(mom.cpu().numpy(), want_mom), k
                for got_c, got_v, passes in ((den, var, 5), (den2, var2, QUALITY_PASSES)):
                    want_c, want_var = V.run_variance(want_out, 1, g, want_mom, passes=passes)
                    assert same(got_c.cpu().numpy()[..., :3], want_c) and same(got_v.cpu().numpy(), want_var), (k, passes)
    finally:
        rdr.close()
    hit = g["tri"] != D.MISS
    tm = {name: V.mse_tm(img, seq["ref"], hit) for name, img in (("temporal", out.cpu().numpy()[..., :3]),
                                                                ("variance, 2 passes", den2.cpu().numpy()[..., :3]),
                                                                ("variance, 5 passes", den.cpu().numpy()[..., :3]))}
    print("tone-mapped MSE over the hit pixels: " + ", ".join(f"{k} {v:.6f}" for k, v in tm.items()))
    assert tm["variance, 2 passes"] < tm["temporal"]
