"""GPU: the guided upsampler (include/srt_upsample.h, srt_amd.upsample.Upsampler) against the independent numpy
float32 restatement of its contract (tests/upsample_ref.py, which never calls into the library), bit for bit, float
output and sRGB8 both.

bits_equal treats any NaN as equal to any NaN.  The synthetic inputs are tests/upsample_cases.py's (the CPU test
tests/test_upsample_ref.py asserts that they take all three paths); the Rubik references (oracle frames, oracle hits,
restated stage and filter) are computed once per process and left unchanged.
"""
import ctypes as C

import numpy as np
import pytest

import denoise_ref as D
import srt_amd as S
import upsample_cases as UC
import upsample_ref as U
from conftest import bits_equal
from test_gpu_denoise import srgb8

pytestmark = pytest.mark.gpu

DEFAULTS = dict(normal_squarings=5, sigma_depth=0.2)
DENOISE_DEFAULTS = dict(passes=5, normal_squarings=5, sigma_color=3.0, sigma_depth=0.2)


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


def to_dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def hits_dev(torch, hits):
    return torch.from_numpy(hits.view(np.int32).reshape(-1, 8).copy()).cuda()


def device_inputs(torch, c):
    return (to_dev(torch, c["accum"]), hits_dev(torch, UC.hit_records(*c["low_parts"], c["rng"])),
            hits_dev(torch, UC.hit_records(*c["full_parts"], c["rng"])))


def want_srgb8(f32):
    h, w = f32.shape[:2]
    want = np.full((h, w, 4), 255, np.uint8)
    want[..., :3] = np.reshape([srgb8(v) for v in f32[..., :3].reshape(-1)], (h, w, 3))
    return want


@pytest.mark.parametrize("w,h,f", UC.CASES)
@pytest.mark.parametrize("frames", [1, 3])
def test_synthetic_bit_exact(torch, w, h, f, frames):
    from srt_amd.upsample import Upsampler

    c = UC.synthetic(w, h, f, frames=frames)
    want, path = U.upsample(c["accum"], frames, c["low"], c["full"], f)
    acc, low, full = device_inputs(torch, c)
    with Upsampler(w, h, f) as up:
        assert up.params == pytest.approx(DEFAULTS) and up.get_int("launches") == 0
        got, got8 = up.run(acc, frames, low, full, srgb=True)
        again = up.run(acc, frames, low, full)          # a second run on the same object: the same bits
        up.synchronize()
        launches = up.get_int("launches")
        ints = {n: up.get_int(n) for n in ("factor", "low.width", "low.height", "width", "height", "scratch.bytes",
                                           "launch.blocks", "launch.block")}
    got, got8, again = got.cpu().numpy(), got8.cpu().numpy(), again.cpu().numpy()
    bad = ~bits_equal(got[..., :3], want)
    print(f"{w}x{h} f={f} frames {frames}: {int(bad.sum())} components differ; paths "
          f"{[int((path == p).sum()) for p in (U.BILINEAR, U.RING, U.NEAREST)]}")
    assert tuple(got.shape) == (f * h, f * w, 4)
    assert not bad.any()
    assert (got[..., 3] == 1.0).all()
    assert (got.view(np.uint32) == again.view(np.uint32)).all()
    assert (got8 == want_srgb8(got)).all()
    header = (UC_ROOT() / "include" / "srt_upsample.h").read_text()
    import re
    assert launches == int(re.search(r"#define\s+SRT_UPSAMPLE_LAUNCHES\s+(\d+)", header).group(1))
    assert ints == {"factor": f, "low.width": w, "low.height": h, "width": f * w, "height": f * h, "scratch.bytes": 0,
                    "launch.blocks": -(-f * w // 32) * -(-f * h // 8), "launch.block": 256}


def UC_ROOT():
    from conftest import ROOT
    return ROOT


@pytest.mark.parametrize("w,h,f", UC.BIG)
def test_nonfinite_colours(torch, w, h, f):
    """NaN / +-Inf low pixels: never part of an average, and the nearest path hands a NaN low pixel through."""
    from srt_amd.upsample import Upsampler

    c = UC.synthetic(w, h, f, nonfinite=True)
    want, path = U.upsample(c["accum"], c["frames"], c["low"], c["full"], f)
    assert path[2 * f, 2 * f] == U.NEAREST and np.isnan(want[2 * f, 2 * f, 0])
    acc, low, full = device_inputs(torch, c)
    with Upsampler(w, h, f) as up:
        got, got8 = up.run(acc, c["frames"], low, full, srgb=True)
        up.synchronize()
    got, got8 = got.cpu().numpy(), got8.cpu().numpy()
    assert bits_equal(got[..., :3], want).all()
    assert np.isnan(got[2 * f, 2 * f, 0]) and got[2 * f, 2 * f, 1] == want[2 * f, 2 * f, 1]
    assert np.isfinite(got[..., :3][path != U.NEAREST]).all()
    assert (got8 == want_srgb8(got)).all()


def test_other_parameters_and_argument_checks(torch):
    """normal_squarings 0 and 8 and sigma_depth 0.01 on 23x14 f=3; a refused set_params leaves the state unchanged; the
    argument checks of run on a live object; unknown get_int names."""
    from srt_amd import _lib
    from srt_amd.upsample import Upsampler

    w, h, f = 23, 14, 3
    c = UC.synthetic(w, h, f, seed=3)
    acc, low, full = device_inputs(torch, c)
    with Upsampler(w, h, f) as up:
        for nsq, sd in ((0, 0.2), (8, 0.2), (5, 0.01), (8, 0.01)):
            up.set_params(normal_squarings=nsq, sigma_depth=sd)
            got = up.run(acc, c["frames"], low, full)
            up.synchronize()
            want, _ = U.upsample(c["accum"], c["frames"], c["low"], c["full"], f, nsq, sd)
            assert bits_equal(got.cpu().numpy()[..., :3], want).all(), (nsq, sd)
        state = up.params
        for bad in (dict(normal_squarings=9), dict(sigma_depth=0.0), dict(sigma_depth=-1.0), dict(sigma_depth=float("nan")),
                    dict(sigma_depth=float("inf"))):
            with pytest.raises(S.SrtError) as e:
                up.set_params(**bad)
            assert e.value.code == _lib.SRT_ERR_INVALID
            assert up.params == state
        with pytest.raises(TypeError):
            up.set_params(sigma_color=1.0)       # there is no colour weight
        for name in ("passes", "tile.max_step", "", "Factor"):
            with pytest.raises(S.SrtError) as e:
                up.get_int(name)
            assert e.value.code == _lib.SRT_ERR_NOT_FOUND
        run = _lib.lib().srt_upsample_run
        o = torch.empty((f * h, f * w, 4), dtype=torch.float32, device="cuda")
        P = lambda t, off=0: C.c_void_p(t.data_ptr() + off)  # noqa: E731
        inv = _lib.SRT_ERR_INVALID
        assert run(up.handle, P(acc), 0, P(low), P(full), P(o), None) == inv          # frames < 1
        assert run(up.handle, P(acc), -2, P(low), P(full), P(o), None) == inv
        assert run(up.handle, P(acc), 3, P(low), P(full), None, None) == inv          # both outputs NULL
        assert run(up.handle, None, 3, P(low), P(full), P(o), None) == inv
        assert run(up.handle, P(acc), 3, None, P(full), P(o), None) == inv
        assert run(up.handle, P(acc), 3, P(low), None, P(o), None) == inv
        assert run(up.handle, P(acc, 4), 3, P(low), P(full), P(o), None) == inv       # misaligned
        assert run(up.handle, P(acc), 3, P(low, 8), P(full), P(o), None) == inv
        assert run(up.handle, P(acc), 3, P(low), P(full, 4), P(o), None) == inv
        assert run(up.handle, P(acc), 3, P(low), P(full), P(o, 8), None) == inv
        assert run(up.handle, P(acc), 3, P(low), P(full), None, P(o, 2)) == inv
        assert run(up.handle, P(acc), 3, P(low), P(full), None, P(o)) == _lib.SRT_OK  # either output alone
        up.synchronize()
    with pytest.raises(RuntimeError):
        up.get_int("factor")                     # closed by the context manager


def test_enqueue_only_on_a_callers_stream(torch):
    """Runs on a caller's stream allocate nothing, and the object holds no device memory."""
    from srt_amd import _lib
    from srt_amd.upsample import Upsampler

    w, h, f = 18, 11, 4
    c = UC.synthetic(w, h, f, seed=9)
    stream = torch.cuda.Stream()
    with Upsampler(w, h, f, stream=stream) as up:
        assert int(_lib.lib().srt_upsample_stream(up.handle)) == stream.cuda_stream
        with torch.cuda.stream(stream):
            acc, low, full = device_inputs(torch, c)
            o1 = torch.empty((f * h, f * w, 4), dtype=torch.float32, device="cuda")
            o2 = torch.empty_like(o1)
            stream.synchronize()
            mem = torch.cuda.memory_allocated()
            for o in (o1, o2):
                assert _lib.lib().srt_upsample_run(up.handle, C.c_void_p(acc.data_ptr()), c["frames"], C.c_void_p(low.data_ptr()),
                                                   C.c_void_p(full.data_ptr()), C.c_void_p(o.data_ptr()), None) == _lib.SRT_OK
            assert torch.cuda.memory_allocated() == mem and up.get_int("scratch.bytes") == 0
        stream.synchronize()
        r1, r2 = o1.cpu().numpy(), o2.cpu().numpy()
    want, _ = U.upsample(c["accum"], c["frames"], c["low"], c["full"], f)
    assert (r1.view(np.uint32) == r2.view(np.uint32)).all() and bits_equal(r1[..., :3], want).all()


CHILD = r"""
import json, sys
import numpy as np
sys.path[:0] = [{tests!r}, {pkg!r}, {root!r}]
import torch
import test_gpu_upsample as T
import upsample_cases as UC
import upsample_ref as U
from conftest import bits_equal
from srt_amd.upsample import Upsampler
res = {{}}
for (w, h, f) in UC.CASES:
    c = UC.synthetic(w, h, f, nonfinite=w >= 10)
    want, _ = U.upsample(c["accum"], c["frames"], c["low"], c["full"], f)
    acc, low, full = T.device_inputs(torch, c)
    with Upsampler(w, h, f) as up:
        got = up.run(acc, c["frames"], low, full)
        up.synchronize()
    res[f"{{w}}x{{h}}x{{f}}"] = int((~bits_equal(got.cpu().numpy()[..., :3], want)).sum())
print("RESULT " + json.dumps(res))
"""


@pytest.mark.parametrize("knob", ["0", "1"])
def test_both_kernel_variants_in_a_child_process(knob):
    """SRT_UPSAMPLE_STAGED=0: every tap is read from global memory; =1: the footprint is staged in LDS.  Both equal the
    restatement on every synthetic case, non-finite colours included."""
    import json
    import os
    import subprocess
    import sys

    from conftest import ROOT

    env = dict(os.environ, SRT_UPSAMPLE_STAGED=knob)
    code = CHILD.format(tests=str(ROOT / "tests"), pkg=str(ROOT / "simple-ray-tracer_amd"), root=str(ROOT))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    res = json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
    print(res)
    assert res == {f"{w}x{h}x{f}": 0 for (w, h, f) in UC.CASES}


def test_end_to_end_on_rubik(torch):
    """Compute renders Rubik at 32 x 24 and 4 spp, Query.closest of primary_rays gives the guides at 32 x 24 and 64 x 48,
    Upsampler.run is followed by Denoiser.run(frames=1).  Both images equal, bit for bit, the oracle's 32 x 24 frame and
    the oracle's closest hits through upsample_ref and then denoise_ref.  Quality, on those bit-identical frames: over the
    hit pixels the upsampled frame is closer to the oracle's 256-spp frame after x / (1 + x) than the same low frame
    replicated 2 x 2 (on the CPU, tools/upsample_grid.py: 0.007233 against 0.011171)."""
    import surface_scenes as SS
    from srt_amd import render as R
    from srt_amd.denoise import Denoiser
    from srt_amd.query import Query
    from srt_amd.upsample import Upsampler

    c = UC.scene_case("rubik")
    low_setup, fullc = c["low_setup"], c["full"]
    w, h, f = low_setup.width, low_setup.height, UC.FACTOR
    W, H = f * w, f * h
    assert (W, H) == (fullc["setup"].width, fullc["setup"].height) == (64, 48)
    rdr = R.Renderer(low_setup, device=0)
    try:
        rdr.render(UC.LOW_SPP)
        rdr.finish()
        frames = rdr.accum_frames
        assert frames == c["low_frames"]
        acc_ptr, _ = rdr.compute.image_pointers()
        with Denoiser(w, h) as dl, Denoiser(W, H) as dn, Query(low_setup.scene) as q, Upsampler(w, h, f) as up:
            q.set_bvh_count(low_setup.bvh_count)
            low_hits = q.closest(dl.primary_rays(low_setup.camera))
            full_hits = q.closest(dn.primary_rays(low_setup.camera))
            ups = up.run(acc_ptr, frames, low_hits, full_hits)
            den = dn.run(ups, 1, full_hits)
            dn.synchronize()
            ups, den = ups.cpu().numpy(), den.cpu().numpy()
            lh, fh = low_hits.numpy(), full_hits.numpy()
    finally:
        rdr.close()
    assert (lh["triangle"] == c["low_hits"]["triangle"]).all() and bits_equal(lh["t"], c["low_hits"]["t"]).all()
    assert (fh["triangle"] == fullc["hits"]["triangle"]).all() and bits_equal(fh["t"], fullc["hits"]["t"]).all()
    want_up, path = U.upsample(c["low_acc"], c["low_frames"], c["low_guide"], fullc["guide"], f)
    accum_up = np.ones((H, W, 4), np.float32)
    accum_up[..., :3] = want_up
    want_den = D.atrous(D.mean_colour(accum_up, 1), fullc["guide"], **DENOISE_DEFAULTS)
    print(f"upsampled: {int((~bits_equal(ups[..., :3], want_up)).sum())} components differ, denoised: "
          f"{int((~bits_equal(den[..., :3], want_den)).sum())}; paths {[int((path == p).sum()) for p in (0, 1, 2)]}")
    assert bits_equal(ups[..., :3], want_up).all() and (ups[..., 3] == 1.0).all()
    assert bits_equal(den[..., :3], want_den).all()
    hit = fullc["guide"]["tri"] != D.MISS
    replicated = U.replicate(D.mean_colour(c["low_acc"], c["low_frames"]), f)
    m_up, m_rep = SS.mse_tm(ups[..., :3], fullc["ref"], hit), SS.mse_tm(replicated, fullc["ref"], hit)
    print(f"x/(1+x) MSE over {int(hit.sum())} hit pixels: upsampled {m_up:.6f}, replicated {m_rep:.6f}")
    assert m_up < m_rep
