"""GPU: the denoiser (include/srt_denoise.h, srt_amd.denoise.Denoiser) against the independent numpy float32
restatement of its filter (tests/denoise_ref.py, which never calls into the library), bit for bit.

bits_equal treats any NaN as equal to any NaN.  The Rubik references (oracle frames, oracle hits, restated
filter) are computed once per module and left unchanged.
"""
import ctypes as C
import json
import os
import pathlib
import subprocess
import sys

import numpy as np
import pytest

import denoise_ref as D
import srt_amd as S
from srt_amd import render as R
from conftest import OBJECTS, ROOT, bits_equal, oracle_render
from oracle import pyoracle as O

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (5, 1), (37, 23), (70, 41)]
DEFAULTS = dict(passes=5, normal_squarings=5, sigma_color=3.0, sigma_depth=0.2)


@pytest.fixture(scope="module")
def torch():
    import torch as t
    return t


def synthetic(w, h, seed=11, nonfinite=False):
    """Random colour (as a sum over 3 frames) and a hand-built guide: misses (a block and scattered ones), two
    bvh values, random unit normals with runs of equal and of opposed ones, equal / near / very different t."""
    rng = np.random.default_rng(seed + 1000 * w + h)
    accum = np.ones((h, w, 4), np.float32)
    accum[..., :3] = rng.uniform(0, 6, (h, w, 3)).astype(np.float32)
    tri = rng.integers(0, 500, (h, w)).astype(np.uint32)
    tri[rng.uniform(size=(h, w)) < 0.15] = D.MISS
    if w >= 10 and h >= 10:
        tri[h // 2:h // 2 + 3, w // 3:w // 3 + 4] = D.MISS
    n = rng.normal(size=(h, w, 3))
    n = (n / np.linalg.norm(n, axis=-1, keepdims=True)).astype(np.float32)
    n[(np.arange(h) % 3) != 0] = n[0, 0]            # two rows in three share one normal
    n[:, (np.arange(w) % 7) == 3] = -n[0, 0]        # columns of the opposed normal
    t = rng.choice(np.asarray([3.0, 3.0, 3.0, 3.02, 3.3, 250.0], np.float32), (h, w))
    bvh = (rng.uniform(size=(h, w)) < 0.25).astype(np.uint32)
    bvh[:, w // 2:] |= (rng.uniform(size=(h, w - w // 2)) < 0.5).astype(np.uint32)
    if w == 1 and h == 1:
        tri[0, 0], bvh[0, 0] = 7, 1
    if nonfinite:
        assert w >= 20 and h >= 20
        accum[3, 4, 0] = np.nan
        accum[10, 11, :3] = np.inf
        accum[h - 1, w - 1, 2] = -np.inf
        accum[15, 2, 1] = np.nan
        # a NaN centre whose neighbours are all rejected: the only pixel of its bvh record in reach of step 1
        tri[6, 20], bvh[6, 20] = 9, 5
        accum[6, 20, :3] = (np.nan, 1.0, 2.0)
        # and a finite centre next to a NaN one with everything else around it a miss
        tri[15:20, 14:19] = D.MISS
        tri[17, 16], tri[17, 17] = 3, 4
        bvh[17, 16] = bvh[17, 17] = 0
        n[17, 16] = n[17, 17]
        accum[17, 17, :3] = (np.nan, np.nan, np.nan)
    hits = np.zeros(w * h, HIT())
    hits["triangle"], hits["t"], hits["normal"], hits["bvh"] = tri.reshape(-1), t.reshape(-1), n.reshape(-1, 3), bvh.reshape(-1)
    hits["material"] = rng.integers(0, 9, w * h)  # never read by the filter
    return accum, hits, D.make_guide(tri, t, n, bvh)


def HIT():
    from srt_amd.query import HIT_DTYPE
    return HIT_DTYPE


def to_dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def hits_dev(torch, hits):
    return torch.from_numpy(hits.view(np.int32).reshape(-1, 8).copy()).cuda()


def gpu_filter(torch, accum, frames, hits, **params):
    from srt_amd.denoise import Denoiser

    h, w = accum.shape[:2]
    with Denoiser(w, h) as dn:
        dn.set_params(**params)
        out = dn.run(to_dev(torch, accum), frames, hits_dev(torch, hits))
        dn.synchronize()
        return out.cpu().numpy(), dn.get_int("launches"), dn.get_int("tile.max_step")


@pytest.mark.parametrize("w,h", SIZES)
def test_synthetic_bit_exact(torch, w, h):
    """1x1, 5x1, 37x23 (no tile multiple, narrower than step 16's reach of 64: both borders clip one pixel's
    taps) and 70x41 (several tiles, both kernels: step 1 tiled, steps 2-16 direct by default)."""
    accum, hits, guide = synthetic(w, h)
    C0 = D.mean_colour(accum, 3)
    for passes in (1, 3, 5):
        got, launches, max_step = gpu_filter(torch, accum, 3, hits, passes=passes, normal_squarings=5, sigma_color=1.0,
                                             sigma_depth=0.05)
        want = D.atrous(C0, guide, passes, 5, 1.0, 0.05)
        print(f"{w}x{h} passes {passes}: {int((~bits_equal(got[..., :3], want)).sum())} components differ")
        assert launches == passes and max_step == 1
        assert bits_equal(got[..., :3], want).all()
        assert (got[..., 3] == 1.0).all()
    hit = guide["tri"] != D.MISS
    if hit.sum() > 20:
        assert (~bits_equal(want[hit], C0[hit])).mean() > 0.5  # the reference itself filters: not the identity


def test_other_parameters_and_srgb_output(torch):
    """normal_squarings 0 and 8, sigmas off the defaults; and the sRGB8 image is the float image's encoding
    (the contract's linear -> sRGB8 with the oracle's pow)."""
    from srt_amd.denoise import Denoiser

    accum, hits, guide = synthetic(37, 23, seed=3)
    C0 = D.mean_colour(accum, 2)
    for nsq, sc, sd in ((0, 0.3, 0.2), (8, 3.0, 0.01)):
        got, _, _ = gpu_filter(torch, accum, 2, hits, passes=4, normal_squarings=nsq, sigma_color=sc, sigma_depth=sd)
        assert bits_equal(got[..., :3], D.atrous(C0, guide, 4, nsq, sc, sd)).all()
    with Denoiser(37, 23) as dn:
        assert dn.params == pytest.approx(DEFAULTS)
        f32, u8 = dn.run(to_dev(torch, accum), 2, hits_dev(torch, hits), srgb=True)
        dn.synchronize()
        f32, u8 = f32.cpu().numpy(), u8.cpu().numpy()
        # rejected parameters leave the state unchanged
        for bad in (dict(passes=9), dict(normal_squarings=9), dict(sigma_color=0.0), dict(sigma_depth=float("nan")),
                    dict(sigma_color=float("inf"))):
            with pytest.raises(S.SrtError) as e:
                dn.set_params(**bad)
            assert e.value.code == 1
        assert dn.params == pytest.approx(DEFAULTS)
        # argument checks of run on a live object
        from srt_amd import _lib
        a, hd, o = to_dev(torch, accum), hits_dev(torch, hits), torch.empty((23, 37, 4), dtype=torch.float32, device="cuda")
        run = _lib.lib().srt_denoise_run
        P = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
        assert run(dn.handle, P(a), 0, P(hd), P(o), None) == _lib.SRT_ERR_INVALID      # frames < 1
        assert run(dn.handle, P(a), 2, None, P(o), None) == _lib.SRT_ERR_INVALID       # no guide, passes > 0
        assert run(dn.handle, P(a), 2, P(hd), None, None) == _lib.SRT_ERR_INVALID      # both outputs NULL
        assert run(dn.handle, None, 2, P(hd), P(o), None) == _lib.SRT_ERR_INVALID
        assert run(dn.handle, P(a), 2, P(hd), None, P(o)) == _lib.SRT_OK               # either output alone
        dn.synchronize()
    assert bits_equal(f32[..., :3], D.atrous(C0, guide, **DEFAULTS)).all()
    want8 = np.full((23, 37, 4), 255, np.uint8)
    want8[..., :3] = np.reshape([srgb8(v) for v in f32[..., :3].reshape(-1)], (23, 37, 3))
    print("sRGB8 components that differ:", int((want8 != u8).sum()))
    assert (u8 == want8).all()


def srgb8(x):
    """device_common.hpp's to_unorm8(linearToSrgb(x)) in scalar float32 with the oracle's pow (contract A: the
    existing parity tests hold the renderer's sRGB8 image bit-identical to it)."""
    x = np.float32(x)
    if np.isnan(x):
        return 0
    e = x * np.float32(12.92) if x < np.float32(0.0031308) else \
        np.float32(1.055) * np.float32(O.pow(x, np.float32(1.0) / np.float32(2.4))) - np.float32(0.055)
    return int(np.rint(np.clip(np.float32(e), np.float32(0), np.float32(1)) * np.float32(255.0)))


def test_nonfinite_colours(torch):
    accum, hits, guide = synthetic(37, 23, seed=5, nonfinite=True)
    C0 = D.mean_colour(accum, 3)
    assert not np.isfinite(C0[6, 20]).all() and (guide["bvh"] == 5).sum() == 1
    for passes in (1, 5):
        got, _, _ = gpu_filter(torch, accum, 3, hits, passes=passes, normal_squarings=2, sigma_color=1.0, sigma_depth=0.2)
        want = D.atrous(C0, guide, passes, 2, 1.0, 0.2)
        assert bits_equal(got[..., :3], want).all()
        assert not np.isnan(got[..., :3][np.isfinite(want)]).any()
        # the lone NaN centre keeps its colour; NaN never spreads into a finite neighbour
        assert bits_equal(got[6, 20, :3], C0[6, 20]).all()
        assert np.isfinite(want[17, 16]).all() and np.isfinite(got[17, 16, :3]).all()
        assert np.isfinite(want).sum() >= np.isfinite(C0).sum()


CHILD = r"""
import json, sys
import numpy as np
sys.path[:0] = [{tests!r}, {pkg!r}, {root!r}]
import torch
import test_gpu_denoise as T
import denoise_ref as D
from conftest import bits_equal
res = {{}}
for (w, h) in ((37, 23), (70, 41)):
    accum, hits, guide = T.synthetic(w, h)
    got, launches, max_step = T.gpu_filter(torch, accum, 3, hits, passes=5, normal_squarings=5, sigma_color=1.0,
                                           sigma_depth=0.05)
    want = D.atrous(D.mean_colour(accum, 3), guide, 5, 5, 1.0, 0.05)
    res[f"{{w}}x{{h}}"] = [int((~bits_equal(got[..., :3], want)).sum()), launches, max_step]
print("RESULT " + json.dumps(res))
"""


@pytest.mark.parametrize("knob,max_step", [("0", 0), ("8", 8)])
def test_forced_paths_in_a_child_process(knob, max_step):
    """SRT_DENOISE_TILE=0: every pass reads its taps from global memory; =8: steps 1-8 take the LDS-tiled kernel
    (step 16 cannot: its halo does not fit the LDS).  Both equal the restatement."""
    env = dict(os.environ, SRT_DENOISE_TILE=knob)
    code = CHILD.format(tests=str(ROOT / "tests"), pkg=str(ROOT / "simple-ray-tracer_amd"), root=str(ROOT))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    res = json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
    print(res)
    assert res == {"37x23": [0, 5, max_step], "70x41": [0, 5, max_step]}


@pytest.fixture(scope="module")
def rubik():
    return S.load_obj(OBJECTS / "Rubik" / "Rubik.obj")


def test_passes_zero_is_the_renderers_output_stage(torch, rubik):
    """Reset + 2 frames of Rubik at 64x48 (accumFrames = 3): with passes = 0 the sRGB8 image equals the
    context's image0 bit for bit and the float image is accum / 3; no guide is needed."""
    from srt_amd.denoise import Denoiser

    setup = R.make_setup(64, 48, show_model=True, models=[rubik])
    rdr = R.Renderer(setup, device=0)
    try:
        rdr.render(2)
        rdr.finish()
        assert rdr.accum_frames == 3
        acc, out = rdr.accum(), rdr.output()
        acc_ptr, _ = rdr.compute.image_pointers()
        with Denoiser(64, 48) as dn:
            dn.set_params(passes=0)
            f32, u8 = dn.run(acc_ptr, 3, None, srgb=True)   # the context's own device image, by pointer
            dn.synchronize()
            assert dn.get_int("launches") == 1 and dn.get_int("passes") == 0
            f32, u8 = f32.cpu().numpy(), u8.cpu().numpy()
    finally:
        rdr.close()
    assert (u8 == out).all()
    assert bits_equal(f32[..., :3], acc[..., :3] / np.float32(3)).all() and (f32[..., 3] == 1.0).all()
    assert (out[..., :3] != 0).mean() > 0.2


def check_closest(scene, bvh_count, rays, hits):
    """Every field of the library's HIT_DTYPE records against the oracle (one BVH record: bvh == 0)."""
    tri_o, t_o, n_o, st = O.Oracle(scene).trace_closest(bvh_count, rays)
    assert st["stack_overflow"] == 0
    assert (hits["triangle"] == tri_o).all(), f"{(hits['triangle'] != tri_o).sum()} triangles differ"
    assert bits_equal(hits["t"], t_o).all()
    assert bits_equal(hits["normal"], n_o).all()
    hit = tri_o != D.MISS
    assert (hits["material"][hit] == scene.tris["mat"][tri_o[hit]]).all()
    assert (hits["bvh"] == 0).all()
    miss = ~hit
    assert bits_equal(hits["t"][miss], rays["t"][miss]).all()
    assert (hits["normal"][miss].view(np.uint32) == 0).all()
    assert (hits["material"][miss] == 0).all() and (hits["pad"] == 0).all()
    return tri_o


def test_primary_rays_and_guide(torch, rubik):
    """Rubik's default camera at 37x23: the rays equal the numpy restatement of tools/bench_queries.py's
    camera_rays bit for bit, and their closest hits equal the oracle's."""
    from srt_amd.denoise import Denoiser
    from srt_amd.query import Query

    w, h = 37, 23
    setup = R.make_setup(w, h, show_model=True, models=[rubik])
    cam = setup.camera
    o, d = D.camera_rays(cam.getOrigin(), cam.getForward(), cam.getRightVector(), cam.getUpVector(), w, h)
    want = np.zeros(w * h, S.RAY_DTYPE)
    want["o"], want["d"], want["t"] = o, d, np.float32(1e30)
    with Denoiser(w, h) as dn, Query(setup.scene) as q:
        q.set_bvh_count(setup.bvh_count)
        rays = dn.primary_rays(cam)
        assert rays.is_cuda and tuple(rays.shape) == (w * h, 8) and rays.dtype == torch.float32
        hits = q.closest(rays).numpy()
        got = rays.cpu().numpy().view(S.RAY_DTYPE).reshape(-1)
    assert (got.view(np.uint32) == want.view(np.uint32)).all()
    # row 0 is the bottom row: the direction's component along `up` grows with j
    up = np.asarray(cam.getUpVector(), np.float32)
    assert (got["d"][(h - 1) * w] @ up) > (got["d"][0] @ up)
    tri_o = check_closest(setup.scene, setup.bvh_count, want, hits)
    hit = tri_o != D.MISS
    assert hit.mean() >= 0.10 and (~hit).mean() >= 0.10  # the oracle alone


@pytest.fixture(scope="module")
def rubik_4spp(rubik):
    """Oracle only: the 4-spp and 256-spp frames of Rubik at 64x48, the oracle's hits of the pixel-centre rays,
    and the restated filter with the default parameters."""
    w, h = 64, 48
    setup = R.make_setup(w, h, show_model=True, models=[rubik])
    cam = setup.camera
    o, d = D.camera_rays(cam.getOrigin(), cam.getForward(), cam.getRightVector(), cam.getUpVector(), w, h)
    rays = np.zeros(w * h, S.RAY_DTYPE)
    rays["o"], rays["d"], rays["t"] = o, d, np.float32(1e30)
    tri, t, nrm, _ = O.Oracle(setup.scene).trace_closest(setup.bvh_count, rays)
    guide = D.make_guide(tri.reshape(h, w), t.reshape(h, w), nrm.reshape(h, w, 3))
    ref_acc, _, _ = oracle_render(setup, 256)
    return {"setup": setup, "guide": guide, "ref": D.mean_colour(ref_acc, 257)}


def test_end_to_end_on_rubik(torch, rubik_4spp):
    """Render 4 spp on the GPU, trace the guide on the GPU, filter with the default parameters: the result equals
    the restatement applied to the read-back accumulation and the oracle's hits, and over hit pixels it is closer
    to the 256-spp frame than the raw mean is (on the CPU, oracle + restatement: 0.4612 against 0.4998)."""
    from srt_amd.denoise import Denoiser
    from srt_amd.query import Query

    setup, guide, ref = rubik_4spp["setup"], rubik_4spp["guide"], rubik_4spp["ref"]
    w, h = setup.width, setup.height
    rdr = R.Renderer(setup, device=0)
    try:
        rdr.render(4)
        rdr.finish()
        frames = rdr.accum_frames
        assert frames == 5
        acc = rdr.accum()
        acc_ptr, _ = rdr.compute.image_pointers()
        with Denoiser(w, h) as dn, Query(setup.scene) as q:
            q.set_bvh_count(setup.bvh_count)
            assert dn.params == pytest.approx(DEFAULTS)
            hits = q.closest(dn.primary_rays(setup.camera))
            got = dn.run(acc_ptr, frames, hits)
            dn.synchronize()
            got = got.cpu().numpy()
            hits = hits.numpy()
            assert dn.get_int("launches") == 5
    finally:
        rdr.close()
    assert (hits["triangle"].reshape(h, w) == guide["tri"]).all() and bits_equal(hits["t"].reshape(h, w), guide["t"]).all()
    noisy = D.mean_colour(acc, frames)
    want = D.atrous(noisy, guide, **DEFAULTS)
    assert bits_equal(got[..., :3], want).all()
    hit = guide["tri"] != D.MISS
    mse = lambda img: float(np.mean((img[hit].astype(np.float64) - ref[hit].astype(np.float64)) ** 2))  # noqa: E731
    print(f"MSE over {int(hit.sum())} hit pixels: denoised {mse(got[..., :3]):.6f}, raw mean {mse(noisy):.6f}")
    assert mse(got[..., :3]) < mse(noisy)


def test_enqueue_only_on_a_callers_stream(torch):
    """Two runs back to back on a caller's stream, read after one synchronise, agree; run allocates nothing."""
    from srt_amd import _lib
    from srt_amd.denoise import Denoiser

    accum, hits, guide = synthetic(70, 41, seed=9)
    stream = torch.cuda.Stream()
    with Denoiser(70, 41, stream=stream) as dn:
        assert dn.get_int("scratch.bytes") == 3 * 16 * 70 * 41
        assert dn.get_int("tile.max_step") == 1 and dn.get_int("tile.lds_bytes") == 36 * 12 * 32
        assert int(_lib.lib().srt_denoise_stream(dn.handle)) == stream.cuda_stream
        with torch.cuda.stream(stream):
            a, hd = to_dev(torch, accum), hits_dev(torch, hits)
            o1 = torch.empty((41, 70, 4), dtype=torch.float32, device="cuda")
            o2 = torch.empty_like(o1)
            stream.synchronize()
            scratch, mem = dn.get_int("scratch.bytes"), torch.cuda.memory_allocated()
            run = _lib.lib().srt_denoise_run
            for o in (o1, o2):
                assert run(dn.handle, C.c_void_p(a.data_ptr()), 3, C.c_void_p(hd.data_ptr()), C.c_void_p(o.data_ptr()),
                           None) == _lib.SRT_OK
            assert torch.cuda.memory_allocated() == mem and dn.get_int("scratch.bytes") == scratch
        stream.synchronize()
        r1, r2 = o1.cpu().numpy(), o2.cpu().numpy()
    assert (r1.view(np.uint32) == r2.view(np.uint32)).all()
    assert bits_equal(r1[..., :3], D.atrous(D.mean_colour(accum, 3), guide, **DEFAULTS)).all()
