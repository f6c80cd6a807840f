"""The denoiser's boundary (include/srt_denoise.h), CPU only: exported symbols, versions, argument checks that
return before any device is touched, the host-side schedule under ASan/UBSan as a stand-alone program, the
numpy restatement of the filter against its own per-pixel form, and the identity of the path tracer's device
code (the new translation unit must not move it)."""
import ctypes as C
import re
import subprocess

import numpy as np

import denoise_ref as D
from conftest import PKG, ROOT


def declared_functions():
    text = (ROOT / "include" / "srt_denoise.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(srt_denoise_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_denoise_symbol():
    names = declared_functions()
    for n in ("srt_denoise_abi_version", "srt_denoise_create", "srt_denoise_destroy", "srt_denoise_stream",
              "srt_denoise_get_int", "srt_denoise_set_params", "srt_denoise_primary_rays", "srt_denoise_run"):
        assert n in names
    for so in ("libsrt_amd.so", "libsrt_amd_F.so"):
        out = subprocess.run(["nm", "-D", "--defined-only", str(PKG / so)], capture_output=True, text=True,
                             check=True).stdout
        exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
        assert not [n for n in names if n not in exported], so


def test_python_binding_and_versions():
    from srt_amd import _lib

    assert set(declared_functions()) == set(_lib.DENOISE_SYMBOLS)
    lib = _lib.lib()
    assert lib.srt_denoise_abi_version() == 1
    assert lib.srt_query_abi_version() == 1 and lib.srt_abi_version() == 2  # the older headers' versions stay
    for n in declared_functions():
        assert isinstance(getattr(lib, n), C._CFuncPtr)
    assert C.sizeof(_lib.DenoiseParams) == 16
    header = (ROOT / "include" / "srt_denoise.h").read_text()
    assert re.search(r"#define\s+SRT_DENOISE_ABI_VERSION\s+1\b", header)
    assert "full" in header.lower() and "band-tiled" in header.lower()  # the stated scope


def test_null_and_range_arguments_without_a_device():
    """Every one of these returns before a device call (this machine may have none: a call that reached the
    device would give SRT_ERR_HIP instead)."""
    from srt_amd import _lib

    lib = _lib.lib()
    inv = _lib.SRT_ERR_INVALID
    p = _lib.DenoiseParams(5, 5, 1.0, 0.05)
    v = C.c_int()
    assert lib.srt_denoise_destroy(None) == inv
    assert lib.srt_denoise_stream(None) is None
    assert lib.srt_denoise_get_int(None, b"passes", C.byref(v)) == inv
    assert lib.srt_denoise_get_params(None, C.byref(p)) == inv
    assert lib.srt_denoise_set_params(None, C.byref(p)) == inv
    assert lib.srt_denoise_primary_rays(None, None, None, None, None, None) == inv
    assert lib.srt_denoise_run(None, None, 1, None, None, None) == inv
    assert lib.srt_denoise_create(0, None, 64, 48, None) == inv
    h = C.c_void_p()
    for w, hgt in ((0, 48), (64, 0), (-1, 48), (64, -7)):
        assert lib.srt_denoise_create(0, None, w, hgt, C.byref(h)) == inv and h.value is None
    for w, hgt in ((65536, 65536), (65536, 1), (1, 65536), (32768, 16384)):  # 2^32 pixels; a dimension; 2^29 pixels
        assert lib.srt_denoise_create(0, None, w, hgt, C.byref(h)) == _lib.SRT_ERR_LIMIT and h.value is None
    assert "2^28" in _lib.last_error()


def _build_host_program(name, extra):
    out = ROOT / "tests" / "cpp" / "_build"
    out.mkdir(exist_ok=True)
    exe = out / name
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-Wall", "-ffp-contract=off", "-I", str(ROOT / "include"),
                    str(ROOT / "tests" / "cpp" / "test_denoise_host.cpp"), str(PKG / "csrc" / "denoise_host.cpp"),
                    "-o", str(exe), *extra], check=True)
    return exe


def test_host_schedule_under_sanitizers():
    """tests/cpp/test_denoise_host.cpp with csrc/denoise_host.cpp linked directly, AddressSanitizer + UBSan, as a
    stand-alone program (host code only: no HIP, no device, nothing preloaded): steps and sigma_color per pass
    exact, the kernel chosen per step, passes = 0, sizing of 1x1 and of a W*H overflow, parameter rejection."""
    exe = _build_host_program("test_denoise_host_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                                                        "-fno-omit-frame-pointer"])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "denoise host checks OK" in r.stdout


def test_code_hash_is_unchanged():
    h = subprocess.run(["make", "-s", "-C", str(PKG), "hash"], capture_output=True, text=True, check=True).stdout.strip()
    stamped = set(re.findall(r'"code_hash"\s*:\s*"([0-9a-f]+)"', (ROOT / "profiles" / "counters.json").read_text()))
    assert stamped == {h}, (stamped, h)


def _synthetic(w, h, seed):
    rng = np.random.default_rng(seed)
    C0 = rng.uniform(0, 2, (h, w, 3)).astype(np.float32)
    tri = rng.integers(0, 50, (h, w)).astype(np.uint32)
    tri[rng.uniform(size=(h, w)) < 0.2] = D.MISS
    n = rng.normal(size=(h, w, 3))
    n = (n / np.linalg.norm(n, axis=-1, keepdims=True)).astype(np.float32)
    n[::2] = n[0, 0]                       # rows of equal normals between the random ones
    n[1, 1:3] = -n[0, 0]                   # and opposed ones
    t = rng.choice(np.asarray([3.0, 3.0, 3.01, 40.0], np.float32), (h, w))
    bvh = (rng.uniform(size=(h, w)) < 0.3).astype(np.uint32)
    return C0, D.make_guide(tri, t, n, bvh)


def test_restatement_matches_its_per_pixel_form():
    """The shifted-array restatement the GPU tests compare with equals the scalar per-pixel loop of the same
    definition bit for bit, NaN and Inf colours included, and it does filter (it is not the identity)."""
    from conftest import bits_equal

    C0, g = _synthetic(13, 9, 5)
    C0[4, 6] = (np.nan, 1.0, 1.0)
    C0[2, 3, 1] = np.inf
    for passes, nsq, sc, sd in ((1, 5, 1.0, 0.05), (3, 0, 0.3, 0.2), (4, 2, 3.0, 0.01)):
        a = D.atrous(C0, g, passes, nsq, sc, sd)
        b = D.atrous_naive(C0, g, passes, nsq, sc, sd)
        assert a.dtype == np.float32 and bits_equal(a, b).all()
        hit = g["tri"] != D.MISS
        assert bits_equal(a[~hit], C0[~hit]).all()          # misses pass through
        assert (~bits_equal(a[hit], C0[hit])).mean() > 0.5  # hits are filtered
    assert bits_equal(D.atrous(C0, g, 0), C0).all()
