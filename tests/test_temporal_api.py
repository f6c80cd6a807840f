"""The temporal reprojection's boundary (include/srt_temporal.h), CPU only: exported symbols, versions, argument
checks that return before any device is touched, the host-side state under ASan/UBSan as a stand-alone program,
the numpy restatement against its own per-pixel form, the meaning of `t` pinned by the oracle's hits, and the
identity of the path tracer's device code (the new translation unit must not move it)."""
import ctypes as C
import re
import subprocess

import numpy as np

import denoise_ref as D
import temporal_ref as T
from conftest import OBJECTS, PKG, ROOT, bits_equal


def declared_functions():
    text = (ROOT / "include" / "srt_temporal.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(srt_temporal_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_temporal_symbol():
    names = declared_functions()
    for n in ("srt_temporal_abi_version", "srt_temporal_create", "srt_temporal_destroy", "srt_temporal_stream",
              "srt_temporal_get_int", "srt_temporal_get_params", "srt_temporal_set_params", "srt_temporal_reset",
              "srt_temporal_accumulate"):
        assert n in names
    for so in ("libsrt_amd.so", "libsrt_amd_F.so"):
        out = subprocess.run(["nm", "-D", "--defined-only", str(PKG / so)], capture_output=True, text=True,
                             check=True).stdout
        exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
        assert not [n for n in names if n not in exported], so


def test_python_binding_and_versions():
    from srt_amd import _lib

    assert set(declared_functions()) == set(_lib.TEMPORAL_SYMBOLS)
    lib = _lib.lib()
    assert lib.srt_temporal_abi_version() == 1
    # the older headers' versions stay
    assert lib.srt_denoise_abi_version() == 1 and lib.srt_query_abi_version() == 1 and lib.srt_abi_version() == 2
    for n in declared_functions():
        assert isinstance(getattr(lib, n), C._CFuncPtr)
    assert C.sizeof(_lib.TemporalParams) == 12 and C.sizeof(_lib.TemporalCamera) == 48
    header = (ROOT / "include" / "srt_temporal.h").read_text()
    assert re.search(r"#define\s+SRT_TEMPORAL_ABI_VERSION\s+1\b", header)
    assert '#include "srt_query.h"' in header
    low = header.lower()
    assert "static" in low and "orthogonal" in low and "srt_denoise_run" in header  # scope, precondition, composition
    from srt_amd.temporal import Temporal  # noqa: F401  (the module imports without a device)


def test_null_and_range_arguments_without_a_device():
    """Every one of these returns before a device call (this machine may have none: a call that reached the
    device would give SRT_ERR_HIP instead)."""
    from srt_amd import _lib

    lib = _lib.lib()
    inv = _lib.SRT_ERR_INVALID
    p = _lib.TemporalParams(32, 0.05, 0.9)
    cam = _lib.TemporalCamera()
    v = C.c_int()
    assert lib.srt_temporal_destroy(None) == inv
    assert lib.srt_temporal_stream(None) is None
    assert lib.srt_temporal_get_int(None, b"frames", C.byref(v)) == inv
    assert lib.srt_temporal_get_params(None, C.byref(p)) == inv
    assert lib.srt_temporal_set_params(None, C.byref(p)) == inv
    assert lib.srt_temporal_reset(None) == inv
    assert lib.srt_temporal_accumulate(None, None, 1, None, C.byref(cam), None) == inv
    assert lib.srt_temporal_create(0, None, 64, 48, None) == inv
    h = C.c_void_p()
    for w, hgt in ((0, 48), (64, 0), (-1, 48), (64, -7)):
        assert lib.srt_temporal_create(0, None, w, hgt, C.byref(h)) == inv and h.value is None
    for w, hgt in ((65536, 65536), (65536, 1), (1, 65536), (32768, 16384)):  # 2^32 pixels; a dimension; 2^29 pixels
        assert lib.srt_temporal_create(0, None, w, hgt, C.byref(h)) == _lib.SRT_ERR_LIMIT and h.value is None
    assert "2^28" in _lib.last_error()


def test_host_state_under_sanitizers():
    """tests/cpp/test_temporal_host.cpp with csrc/temporal_host.cpp linked directly, AddressSanitizer + UBSan, as a
    stand-alone program (host code only: no HIP, no device, nothing preloaded): parameter ranges, sizing of 1x1 and
    of a W*H overflow, the launch grid, and the ping-pong index over calls and resets."""
    out = ROOT / "tests" / "cpp" / "_build"
    out.mkdir(exist_ok=True)
    exe = out / "test_temporal_host_san"
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-Wall", "-ffp-contract=off", "-I", str(ROOT / "include"),
                    str(ROOT / "tests" / "cpp" / "test_temporal_host.cpp"), str(PKG / "csrc" / "temporal_host.cpp"),
                    "-o", str(exe), "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-fno-omit-frame-pointer"], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "temporal host checks OK" in r.stdout


def test_cpp_mirror_compiles():
    """include/srt/temporal.hpp compiles on its own against the C header (syntax only: nothing is linked)."""
    src = ('#include "srt/temporal.hpp"\n'
           "int use(srt::Temporal& t, const srt_temporal_camera& c, void* p, const srt_hit* g) {\n"
           "  t.accumulate(p, 1, g, c, p); t.reset(); t.set_params(t.params()); return t.get_int(\"frames\"); }\n")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", str(ROOT / "include"), "-x", "c++", "-"],
                   input=src, text=True, check=True)


def test_code_hash_is_unchanged():
    h = subprocess.run(["make", "-s", "-C", str(PKG), "hash"], capture_output=True, text=True, check=True).stdout.strip()
    stamped = set(re.findall(r'"code_hash"\s*:\s*"([0-9a-f]+)"', (ROOT / "profiles" / "counters.json").read_text()))
    assert stamped == {h}, (stamped, h)


CAMERAS = [((0, 0, 4), -90, 0), ((0, 0, 4), -90, 0), ((.15, .05, 3.9), -92, 1), ((.3, .1, 3.8), -94, 2),
           ((-.4, 0, 3.8), -84, -1)]


def test_restatement_matches_its_per_pixel_form():
    """The vectorised restatement the GPU tests compare with equals the scalar per-pixel loop of the same definition
    bit for bit over the five cameras of the two-wall scene, NaN and Inf colours included, and it does accumulate."""
    w, h = 13, 9
    rng = np.random.default_rng(3)
    a, b = T.TemporalRef(w, h, max_history=3), T.TemporalRef(w, h, max_history=3)
    seen = set()
    for k, (pos, yaw, pitch) in enumerate(CAMERAS + CAMERAS[:1] * 2):
        cam = T.camera_vectors(pos, yaw, pitch)
        g = D.make_guide(*T.two_wall_guide(cam, w, h))
        accum = np.ones((h, w, 4), np.float32)
        accum[..., :3] = rng.uniform(0, 6, (h, w, 3)).astype(np.float32)
        if k in (0, 2):
            accum[4, 6, :3] = (np.nan, 1.0, 1.0)
            accum[5, 5, 1] = np.inf
            accum[4, 3, 2] = -np.inf
        x, y = a.accumulate(accum, 3, g, cam), b.accumulate(accum, 3, g, cam, naive=True)
        assert x.dtype == np.float32 and bits_equal(x, y).all(), k
        seen |= set(np.unique(x[..., 3]).tolist())
        hit = g["tri"] != D.MISS
        assert hit.sum() > 10 and (x[..., 3][~hit] == 1).all()
    assert seen == {1.0, 2.0, 3.0}


def test_reprojection_identity_on_rubik():
    """Rubik's default camera at 37x23 with the oracle's hits and the same camera twice: every hit pixel's surface
    point reprojects onto its own pixel centre, (uu, vv) = (i, j) within 1e-3, and `a` is its own t.  This pins
    the meaning of t (units of the unnormalised ray direction) independently of the kernel."""
    import srt_amd as S
    from oracle import pyoracle as O
    from srt_amd import render as R

    w, h = 37, 23
    setup = R.make_setup(w, h, show_model=True, models=[S.load_obj(OBJECTS / "Rubik" / "Rubik.obj")])
    cam = T.as_camera(setup.camera)
    o, d = D.camera_rays(*cam, w, h)
    assert bits_equal(d.reshape(h, w, 3), T.pixel_dirs(cam, w, h)).all()  # the two restatements of the rays agree
    rays = np.zeros(w * h, S.RAY_DTYPE)
    rays["o"], rays["d"], rays["t"] = o, d, np.float32(1e30)
    tri, t, _, _ = O.Oracle(setup.scene).trace_closest(setup.bvh_count, rays)
    hit = (tri != D.MISS).reshape(h, w)
    assert hit.mean() >= 0.10
    a, uu, vv = T.reproject(t.reshape(h, w), cam, cam, w, h)
    jj, ii = np.mgrid[0:h, 0:w]
    print("max |uu - i|, |vv - j|, |a/t - 1| over hit pixels:", np.abs(uu - ii)[hit].max(), np.abs(vv - jj)[hit].max(),
          np.abs(a / t.reshape(h, w) - 1)[hit].max())
    assert (np.abs(uu - ii)[hit] < 1e-3).all() and (np.abs(vv - jj)[hit] < 1e-3).all()
    assert (np.abs(a / t.reshape(h, w) - 1)[hit] < 1e-5).all()
