"""Temporal luminance moments and the variance-guided filter (include/srt_variance.h), CPU only: exported symbols,
version and struct size, argument checks that return before any device is touched, the C++ mirrors, the host-side
state and schedule under ASan/UBSan as a stand-alone program, and properties of the numpy restatement alone
(tests/variance_ref.py): its per-pixel forms, the state rules, pins of the definition on hand-made inputs and the
quality comparison on Rubik that tests/test_gpu_variance.py then asserts on the GPU's frames."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import denoise_ref as D
import temporal_motion_ref as M
import temporal_ref as T
import variance_ref as V
import variance_scenes as VS
from conftest import PKG, ROOT, bits_equal

NAMES = ("srt_variance_abi_version", "srt_temporal_enable_moments", "srt_temporal_accumulate_moments",
         "srt_denoise_enable_variance", "srt_denoise_get_var_params", "srt_denoise_set_var_params",
         "srt_denoise_run_variance")
QUALITY_PASSES = 2  # of the quality comparison at 64 x 48 (see test_quality_on_rubik)


def test_library_exports_every_symbol_and_the_header_declares_them():
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "srt_variance.h").read_text(), flags=re.S)
    assert sorted(set(re.findall(r"\b(srt_[a-z0-9_]+)\s*\(", text))) == sorted(NAMES)
    for so in ("libsrt_amd.so", "libsrt_amd_F.so"):
        out = subprocess.run(["nm", "-D", "--defined-only", str(PKG / so)], capture_output=True, text=True, check=True).stdout
        exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
        assert not [n for n in NAMES if n not in exported], so


def test_python_binding_versions_and_size():
    from srt_amd import _lib
    from srt_amd.denoise import Denoiser
    from srt_amd.temporal import Temporal

    assert set(_lib.VARIANCE_SYMBOLS) == set(NAMES)
    for other in (_lib.TEMPORAL_SYMBOLS, _lib.TEMPORAL_MOTION_SYMBOLS, _lib.DENOISE_SYMBOLS):
        assert not set(_lib.VARIANCE_SYMBOLS) & set(other)
    lib = _lib.lib()
    assert lib.srt_variance_abi_version() == 1
    assert (lib.srt_temporal_abi_version(), lib.srt_temporal_motion_abi_version(), lib.srt_denoise_abi_version()) == (1, 1, 1)
    assert C.sizeof(_lib.DenoiseVarParams) == 8
    header = (ROOT / "include" / "srt_variance.h").read_text()
    assert re.search(r"#define\s+SRT_VARIANCE_ABI_VERSION\s+1\b", header)
    assert '#include "srt_temporal_motion.h"' in header and '#include "srt_denoise.h"' in header
    for m in (Temporal.enable_moments, Temporal.accumulate_moments, Denoiser.enable_variance, Denoiser.set_variance_params,
              Denoiser.run_variance):
        assert callable(m)


def test_argument_checks_without_a_device():
    """Each of these returns before a device call (with none here, one that reached a device would give SRT_ERR_HIP)."""
    from srt_amd import _lib

    lib, inv = _lib.lib(), _lib.SRT_ERR_INVALID
    buf = (C.c_float * 64)()
    p = C.c_void_p(C.addressof(buf) & ~15 | 16)
    cam = _lib.TemporalCamera()
    assert lib.srt_temporal_enable_moments(None) == inv
    assert lib.srt_temporal_accumulate_moments(None, p, 1, p, C.byref(cam), p, p) == inv
    assert lib.srt_denoise_enable_variance(None) == inv
    assert lib.srt_denoise_run_variance(None, p, 1, p, p, p, None, None) == inv
    vp = _lib.DenoiseVarParams()
    assert lib.srt_denoise_get_var_params(None, C.byref(vp)) == inv
    good = _lib.DenoiseVarParams(1.0, 4)
    assert lib.srt_denoise_set_var_params(None, C.byref(good)) == inv and "NULL object" in _lib.last_error()
    assert lib.srt_denoise_set_var_params(None, None) == inv and "sigma_lum" in _lib.last_error()
    for sl, mh in ((0.0, 4), (-1.0, 4), (float("nan"), 4), (float("inf"), 4), (1.0, 0), (1.0, 65536), (1.0, 0xFFFFFFFF)):
        bad = _lib.DenoiseVarParams(sl, mh)
        assert lib.srt_denoise_set_var_params(None, C.byref(bad)) == inv and "sigma_lum" in _lib.last_error(), (sl, mh)
    for sl, mh in ((1e-30, 1), (3e38, 65535)):  # valid: the check that answers is the object's
        ok = _lib.DenoiseVarParams(sl, mh)
        assert lib.srt_denoise_set_var_params(None, C.byref(ok)) == inv and "NULL object" in _lib.last_error()


def test_cpp_mirrors_compile():
    """include/srt/temporal.hpp and include/srt/denoise.hpp with the new methods compile against the C headers."""
    src = ('#include "srt/temporal.hpp"\n#include "srt/denoise.hpp"\n'
           "int use(srt::Temporal& t, srt::Denoiser& d, const void* a, const srt_hit* g, const srt_temporal_camera& c, void* o, void* m) {\n"
           "  t.EnableMoments(); t.AccumulateMoments(a, 1, g, c, o, m);\n"
           "  d.EnableVariance(); srt_denoise_var_params p = d.variance_params(); d.SetVarianceParams(p);\n"
           "  d.RunVariance(o, 1, g, m, o, nullptr, nullptr);\n"
           '  return t.get_int("moments.bytes") + d.get_int("variance.bytes") + SRT_VARIANCE_ABI_VERSION; }\n')
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", str(ROOT / "include"), "-x", "c++", "-"],
                   input=src, text=True, check=True)


def test_host_state_under_sanitizers():
    """tests/cpp/test_variance_host.cpp with csrc/temporal_host.cpp and csrc/denoise_host.cpp linked directly,
    AddressSanitizer + UBSan, as a stand-alone program (host code only: no HIP, no device, nothing preloaded)."""
    out = ROOT / "tests" / "cpp" / "_build"
    out.mkdir(exist_ok=True)
    exe = out / "test_variance_host_san"
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-Wall", "-ffp-contract=off", "-I", str(ROOT / "include"),
                    str(ROOT / "tests" / "cpp" / "test_variance_host.cpp"), str(PKG / "csrc" / "temporal_host.cpp"),
                    str(PKG / "csrc" / "denoise_host.cpp"), "-o", str(exe), "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "variance host checks OK" in r.stdout


# ---------------------------------------------------------------------------------------------------------------
# the restatement alone
# ---------------------------------------------------------------------------------------------------------------
def two_wall_run(w, h, with_poses=True, frames=None):
    """The five moving two-wall frames through the restatement: per frame (out, moments, guide)."""
    ref, res = V.VarianceTemporalRef(w, h), []
    for cam, accum, fields, poses in (frames or M.moving_two_wall_frames(w, h)):
        if with_poses:
            ref.set_models(poses)
        g = D.make_guide(*fields)
        res.append(ref.accumulate_moments(accum, 3, g, cam) + (g,))
    return res


@pytest.mark.parametrize("w,h", [(5, 1), (37, 23)])
def test_filter_matches_its_per_pixel_form(w, h):
    """resolve and one_pass equal their scalar per-pixel loops bit for bit on the last two-wall frame, over three
    passes (steps 1, 2, 4); at 37x23 both branches of var_0 are taken."""
    out, mom, g = two_wall_run(w, h)[-1]
    a, b = V.resolve(out, 1, g, mom), V.resolve_naive(out, 1, g, mom)
    assert bits_equal(a[0], b[0]).all() and bits_equal(a[1], b[1]).all()
    C, var = a
    for i in range(3):
        x, y = V.one_pass(C, var, g, 1 << i), V.one_pass_naive(C, var, g, 1 << i)
        assert bits_equal(x[0], y[0]).all() and bits_equal(x[1], y[1]).all(), i
        C, var = x
    if w >= 37:
        hit = g["tri"] != D.MISS
        assert (mom[..., 3][hit] < 4).any() and (mom[..., 3][hit] >= 4).any() and (a[1][hit] > 0).mean() > 0.9


@pytest.mark.parametrize("with_poses", [True, False])
def test_shares_of_the_two_wall_frames(with_poses):
    """The conditions tests/test_gpu_variance.py relies on, on the restatement alone: from 37 wide the fifth frame
    has at least 2% of its hit pixels on the spatial branch (N < 4), at least 50% on the temporal one and at least
    10% of the image a miss; `out` is bit for bit the plain restatement's."""
    for w, h in ((37, 23), (70, 41)):
        plain = M.TemporalMotionRef(w, h)
        frames = M.moving_two_wall_frames(w, h)
        res = two_wall_run(w, h, with_poses, frames)
        for (out, mom, g), (cam, accum, fields, poses) in zip(res, frames):
            if with_poses:
                plain.set_models(poses)
            assert bits_equal(out, plain.accumulate(accum, 3, g, cam)).all()
            assert (mom[..., 3] == out[..., 3]).all()  # moments on every frame: their N is the colour's
        hit = g["tri"] != D.MISS
        n = mom[..., 3][hit]
        print(f"{w}x{h} poses={with_poses}: N < 4 {(n < 4).mean():.3f}, N >= 4 {(n >= 4).mean():.3f}, miss {(~hit).mean():.3f}")
        assert (n < 4).mean() >= 0.02 and (n >= 4).mean() >= 0.50 and (~hit).mean() >= 0.10


def test_state_rules_reset_and_mixed_calls():
    """A plain accumulate between two accumulate_moments leaves the next frame's moments at (L, L*L, 1) while its
    colour keeps its history; reset drops both; the colour output never depends on which call was used."""
    w, h = 37, 23
    frames = M.moving_two_wall_frames(w, h)
    mixed, plain = V.VarianceTemporalRef(w, h), M.TemporalMotionRef(w, h)
    for k, (cam, accum, fields, poses) in enumerate(frames):
        g = D.make_guide(*fields)
        want = plain.accumulate(accum, 3, g, cam)
        if k == 2:
            assert bits_equal(mixed.accumulate(accum, 3, g, cam), want).all() and not mixed.mom_valid
            continue
        out, mom = mixed.accumulate_moments(accum, 3, g, cam)
        assert bits_equal(out, want).all()
        L = V.lum(D.mean_colour(accum, 3))
        if k in (0, 3):  # no history at all; a colour history without moments
            assert bits_equal(mom[..., 0], L).all() and bits_equal(mom[..., 1], L * L).all() and (mom[..., 3] == 1).all()
            assert k == 0 or (out[..., 3] >= 2).mean() > 0.2
        else:
            assert (mom[..., 3] >= 2).mean() > 0.2 and not bits_equal(mom[..., 0], L).all()
    mixed.reset()
    cam, accum, fields, _ = frames[0]
    out, mom = mixed.accumulate_moments(accum, 3, D.make_guide(*fields), cam)
    assert (out[..., 3] == 1).all() and (mom[..., 3] == 1).all() and (mom[..., 2] == 0).mean() > 0.99


def still_frames(w, h, colours):
    """A still camera on the two-wall scene, frame k of constant colour colours[k]."""
    cam = T.camera_vectors((0, 0, 4), -90, 0)
    g = D.make_guide(*T.two_wall_guide(cam, w, h))
    ref, res = V.VarianceTemporalRef(w, h), []
    for c in colours:
        accum = np.ones((h, w, 4), np.float32)
        accum[..., :3] = np.asarray(c, np.float32)
        res.append(ref.accumulate_moments(accum, 1, g, cam))
    return g, res


def test_constant_history_has_zero_variance():
    """Every frame the same colour, its luminance a power of two (so every weighted mean of it is exact): m1 == L,
    m2 == L*L and v == 0 exactly at every pixel of every frame, while N grows on the hit pixels."""
    c = (0.0, 0.0, np.float32(2.0) / V.LB)
    L = V.lum(np.asarray(c, np.float32))
    assert L == np.float32(2.0)
    g, res = still_frames(37, 23, [c] * 5)
    hit = g["tri"] != D.MISS
    for out, mom in res:
        assert (mom[..., 0] == 2).all() and (mom[..., 1] == 4).all() and (mom[..., 2] == 0).all()
    assert (mom[..., 3][M.interior(hit)] == 5).all() and (mom[..., 3][~hit] == 1).all()


def test_alternating_sequence_gives_the_predicted_variance():
    """Grey frames of luminance a, b, a, b: with 1/N weights the moments are the running means, so after four frames
    v = (a - b)^2 / 4 on every interior hit pixel, within 1e-5 relative (a handful of fp32 roundings of values of
    order 1-10); after two frames the same; a miss pixel keeps v == 0."""
    a, b = 1.0, 3.0
    g, res = still_frames(37, 23, [(a,) * 3, (b,) * 3, (a,) * 3, (b,) * 3])
    inner = M.interior(g["tri"] != D.MISS)
    La, Lb = (float(V.lum(np.full(3, x, np.float32))) for x in (a, b))
    want = (La - Lb) ** 2 / 4
    for k in (1, 3):
        mom = res[k][1]
        assert (mom[..., 3][inner] == k + 1).all()
        np.testing.assert_allclose(mom[..., 2][inner], want, rtol=1e-5)
        np.testing.assert_allclose(mom[..., 0][inner], (La + Lb) / 2, rtol=1e-5)
    # three frames: mean (2a + b) / 3, variance 2 (a - b)^2 / 9
    np.testing.assert_allclose(res[2][1][..., 2][inner], 2 * (La - Lb) ** 2 / 9, rtol=1e-5)
    assert (res[3][1][..., 2][g["tri"] == D.MISS] == 0).all()


def test_equal_neighbour_moments_give_zero_spatial_variance():
    """Every pixel young (N = 1) with the same moments (m1, m2) = (2, 4): a = s1/sw and b = s2/sw are exact (powers
    of two times the same sum), so var_0 == 0 exactly on every pixel; with m2 = 5 instead the estimate is
    (5 - 4) * min_history / N = 4 on every hit pixel."""
    w, h = 37, 23
    cam = T.camera_vectors((0, 0, 4), -90, 0)
    g = D.make_guide(*T.two_wall_guide(cam, w, h))
    hit = g["tri"] != D.MISS
    colour = np.ones((h, w, 4), np.float32)
    mom = np.empty((h, w, 4), np.float32)
    mom[...] = (2, 4, 123.0, 1)
    assert (V.resolve(colour, 1, g, mom)[1] == 0).all()
    mom[..., 1] = 5
    var0 = V.resolve(colour, 1, g, mom)[1]
    np.testing.assert_allclose(var0[hit], 4.0, rtol=1e-6)
    assert (var0[~hit] == 0).all()
    mom[..., 3] = 4  # old enough: the temporal variance is taken as it is
    assert (V.resolve(colour, 1, g, mom)[1][hit] == 123.0).all()


def test_quality_on_rubik():
    """Rubik 64x48, the 8-frame orbit and the 8-frame spin, the oracle's 1-spp frames through the restatements against
    the oracle's 256-spp frame, over the hit pixels: MSE of linear radiance | MSE after x/(1+x).
      orbit: raw 0.396853 | 0.018364, temporal 0.087625 | 0.007654, + existing filter 0.117137 | 0.007652,
             + variance-guided, 2 passes 0.107811 | 0.006213; at the default 5 passes 0.167117 | 0.008880
      spin:  raw 2.286032 | 0.013870, temporal 0.134010 | 0.008875, + existing filter 0.120490 | 0.006981,
             + variance-guided, 2 passes 0.129056 | 0.006745; at the default 5 passes 0.158395 | 0.007543
    Asserted: with 2 passes the variance-guided result is strictly closer to the reference than the temporal output it
    was fed, tone-mapped, on both sequences.  At 64 x 48 the steps 4, 8 and 16 of passes 3-5 span much of the cube, and
    at 5 passes the filter is WORSE than its input on the orbit; that, and the comparison with the existing filter,
    are recorded, not asserted."""
    for name, seq in (("orbit", VS.orbit()), ("spin", VS.spin())):
        out, mom = VS.temporal_pass(seq)[-1]
        g = seq["guides"][-1]
        imgs = VS.four_images(seq, out, mom, seq["accs"][-1])
        imgs["variance, 2 passes"] = V.run_variance(out, 1, g, mom, passes=QUALITY_PASSES)[0]
        m = VS.metrics(seq, imgs)
        for k, (lin, tm) in m.items():
            print(f"{name:5} {k:18} mse {lin:.6f}  tone-mapped {tm:.6f}")
        assert m["variance, 2 passes"][1] < m["temporal"][1]
        assert m["temporal"][1] < m["raw"][1]
