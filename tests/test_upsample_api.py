"""The guided upsampler's boundary (include/srt_upsample.h), CPU only: exported symbols, versions, every argument
check that returns before any device is touched (through the C ABI and through the Python object), the host part
under ASan/UBSan as a stand-alone program, and the identity of the path tracer's device code (the new translation
unit must not move it)."""
import ctypes as C
import re
import subprocess

import pytest

from conftest import PKG, ROOT
from srt_amd._lib import UPSAMPLE_SYMBOLS  # noqa: F401  (the binding this file tests)

NAMES = ("srt_upsample_abi_version", "srt_upsample_create", "srt_upsample_destroy", "srt_upsample_stream",
         "srt_upsample_get_int", "srt_upsample_get_params", "srt_upsample_set_params", "srt_upsample_run")
GET_INT_NAMES = ("factor", "low.width", "low.height", "width", "height", "launches", "scratch.bytes", "launch.blocks",
                 "launch.block")


def declared_functions():
    text = (ROOT / "include" / "srt_upsample.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(srt_upsample_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_upsample_symbol():
    assert declared_functions() == sorted(NAMES)
    for so in ("libsrt_amd.so", "libsrt_amd_F.so"):
        out = subprocess.run(["nm", "-D", "--defined-only", str(PKG / so)], capture_output=True, text=True,
                             check=True).stdout
        exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
        assert not [n for n in NAMES if n not in exported], so


def test_python_binding_and_versions():
    from srt_amd import _lib

    assert set(NAMES) == set(_lib.UPSAMPLE_SYMBOLS)
    for other in (_lib.EXPORTED_SYMBOLS, _lib.QUERY_SYMBOLS, _lib.DENOISE_SYMBOLS, _lib.TEMPORAL_SYMBOLS):
        assert not set(_lib.UPSAMPLE_SYMBOLS) & set(other)
    lib = _lib.lib()
    assert lib.srt_upsample_abi_version() == 1
    # additive: the other headers' versions stay
    assert lib.srt_denoise_abi_version() == 1 and lib.srt_query_abi_version() == 1 and lib.srt_abi_version() == 2
    assert lib.srt_temporal_abi_version() == 1
    for n in NAMES:
        assert isinstance(getattr(lib, n), C._CFuncPtr)
    assert C.sizeof(_lib.UpsampleParams) == 8
    header = (ROOT / "include" / "srt_upsample.h").read_text()
    assert re.search(r"#define\s+SRT_UPSAMPLE_ABI_VERSION\s+1\b", header)
    assert re.search(r"#define\s+SRT_UPSAMPLE_LAUNCHES\s+1\b", header)
    for name in GET_INT_NAMES:
        assert f'"{name}"' in header
    assert "band-tiled" in header.lower() and "multiple of the factor" in header.lower()  # the stated scope


def test_null_and_range_arguments_without_a_device():
    """Every one of these returns before a device call (this machine may have none: a call that reached the device
    would give SRT_ERR_HIP instead)."""
    from srt_amd import _lib

    lib = _lib.lib()
    inv, lim = _lib.SRT_ERR_INVALID, _lib.SRT_ERR_LIMIT
    p = _lib.UpsampleParams(5, 0.2)
    v = C.c_int()
    assert lib.srt_upsample_destroy(None) == inv
    assert lib.srt_upsample_stream(None) is None
    assert lib.srt_upsample_get_int(None, b"factor", C.byref(v)) == inv
    assert lib.srt_upsample_get_params(None, C.byref(p)) == inv
    assert lib.srt_upsample_set_params(None, C.byref(p)) == inv
    assert lib.srt_upsample_run(None, None, 1, None, None, None, None) == inv
    assert lib.srt_upsample_create(0, None, 32, 24, 2, None) == inv
    h = C.c_void_p()
    for w, hgt, f in ((0, 24, 2), (32, 0, 2), (-1, 24, 2), (32, -7, 2),          # a dimension < 1
                      (32, 24, 0), (32, 24, 5), (32, 24, -2), (32, 24, 1 << 30)):  # a factor outside 1..4
        assert lib.srt_upsample_create(0, None, w, hgt, f, C.byref(h)) == inv and h.value is None, (w, hgt, f)
    assert "factor" in _lib.last_error()
    # the denoiser's image limits, applied to the FULL size: a dimension past 65535, more than 2^28 pixels
    for w, hgt, f in ((32768, 1, 2), (1, 16384, 4), (21846, 3, 3), (65536, 1, 1), (16384, 8193, 2), (8193, 8192, 2),
                      (2**31 - 1, 2**31 - 1, 4)):
        assert lib.srt_upsample_create(0, None, w, hgt, f, C.byref(h)) == lim and h.value is None, (w, hgt, f)
    assert "2^28" in _lib.last_error()


def test_python_object_refuses_before_a_device():
    import srt_amd as S
    from srt_amd import _lib
    from srt_amd.upsample import Upsampler

    for args, code in (((32, 24, 0), _lib.SRT_ERR_INVALID), ((32, 24, 5), _lib.SRT_ERR_INVALID),
                       ((0, 24, 2), _lib.SRT_ERR_INVALID), ((32, -1, 2), _lib.SRT_ERR_INVALID),
                       ((32768, 1, 2), _lib.SRT_ERR_LIMIT), ((8193, 8192, 2), _lib.SRT_ERR_LIMIT)):
        with pytest.raises(S.SrtError) as e:
            Upsampler(*args)
        assert e.value.code == code, args


def _build_host_program(name, extra):
    out = ROOT / "tests" / "cpp" / "_build"
    out.mkdir(exist_ok=True)
    exe = out / name
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-Wall", "-ffp-contract=off", "-I", str(ROOT / "include"),
                    str(ROOT / "tests" / "cpp" / "test_upsample_host.cpp"), str(PKG / "csrc" / "upsample_host.cpp"),
                    "-o", str(exe), *extra], check=True)
    return exe


def test_host_part_under_sanitizers():
    """tests/cpp/test_upsample_host.cpp with csrc/upsample_host.cpp linked directly, AddressSanitizer + UBSan, as a
    stand-alone program (host code only: no HIP, no device, nothing preloaded): parameter rejection, the plan of every
    factor with its limits, the axis tables, and every tap of a tile inside the staged footprint."""
    exe = _build_host_program("test_upsample_host_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                                                         "-fno-omit-frame-pointer"])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "upsample host checks OK" in r.stdout


def test_cpp_mirror_compiles():
    """include/srt/upsample.hpp compiles on its own against the C header (syntax only: nothing is linked)."""
    src = ('#include "srt/upsample.hpp"\n'
           "int use(srt::Upsampler& u, const void* a, const srt_hit* g, void* o) {\n"
           "  srt::Upsampler v(std::move(u)); v.run(a, 1, g, g, o, nullptr); v.set_params(v.params());\n"
           "  return v.get_int(\"launches\") + (v.stream() != nullptr) + (v.handle() != nullptr); }\n")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", str(ROOT / "include"), "-x", "c++", "-"],
                   input=src, text=True, check=True)


def test_run_refusals_say_why():
    """A refused srt_upsample_run leaves its own text in srt_last_error(), not an earlier call's."""
    from srt_amd import _lib

    lib = _lib.lib()
    h = C.c_void_p()
    assert lib.srt_upsample_create(0, None, 32, 24, 9, C.byref(h)) == _lib.SRT_ERR_INVALID  # leaves "factor ..." behind
    assert lib.srt_upsample_run(None, None, 1, None, None, None, None) == _lib.SRT_ERR_INVALID
    assert "srt_upsample_run" in _lib.last_error() and "factor" not in _lib.last_error()


def test_code_hash_is_unchanged():
    h = subprocess.run(["make", "-s", "-C", str(PKG), "hash"], capture_output=True, text=True, check=True).stdout.strip()
    stamped = set(re.findall(r'"code_hash"\s*:\s*"([0-9a-f]+)"', (ROOT / "profiles" / "counters.json").read_text()))
    assert stamped == {h}, (stamped, h)
