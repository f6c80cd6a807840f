"""The deforming-mesh extension of the temporal reprojection (include/srt_temporal_deform.h) and the surface refit
(include/srt_surface_refit.h), CPU only: exported symbols, versions, every argument check that returns before a
device is touched (with none here, a call that reached one would give SRT_ERR_HIP), the C++ mirrors, and the mesh
bookkeeping under ASan/UBSan as a stand-alone program."""
import ctypes as C
import re
import subprocess

import numpy as np

from conftest import PKG, ROOT

NAMES = ("srt_temporal_deform_abi_version", "srt_temporal_set_mesh", "srt_temporal_set_vertices")
SURFACE_NAMES = ("srt_surface_refit_abi_version", "srt_surface_create_ex", "srt_surface_create_obj_ex", "srt_surface_refit")


def declared(header, prefix):
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / header).read_text(), flags=re.S)
    return sorted(set(re.findall(r"\b(" + prefix + r"[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_symbol():
    from srt_amd import _lib

    assert declared("srt_temporal_deform.h", "srt_temporal_") == sorted(NAMES) == sorted(_lib.TEMPORAL_DEFORM_SYMBOLS)
    assert declared("srt_surface_refit.h", "srt_surface_") == sorted(SURFACE_NAMES) == sorted(_lib.SURFACE_REFIT_SYMBOLS)
    for other in (_lib.TEMPORAL_SYMBOLS, _lib.TEMPORAL_MOTION_SYMBOLS, _lib.VARIANCE_SYMBOLS, _lib.SURFACE_SYMBOLS):
        assert not (set(NAMES) | set(SURFACE_NAMES)) & set(other)
    for so in ("libsrt_amd.so", "libsrt_amd_F.so"):
        out = subprocess.run(["nm", "-D", "--defined-only", str(PKG / so)], capture_output=True, text=True, check=True).stdout
        exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
        assert not [n for n in NAMES + SURFACE_NAMES if n not in exported], so


def test_versions_and_headers():
    from srt_amd import _lib

    lib = _lib.lib()
    assert lib.srt_temporal_deform_abi_version() == 1 and lib.srt_surface_refit_abi_version() == 1
    # the older headers' versions stay
    assert lib.srt_temporal_abi_version() == 1 and lib.srt_temporal_motion_abi_version() == 1 and lib.srt_surface_abi_version() == 1
    td = (ROOT / "include" / "srt_temporal_deform.h").read_text()
    assert re.search(r"#define\s+SRT_TEMPORAL_DEFORM_ABI_VERSION\s+1\b", td) and '#include "srt_temporal_motion.h"' in td
    for word in ("RIGID", "DEFORMING", "bitwise", "denom = 1.0f / (d00*d11 - d01*d01)", "u = (1.0f - v) - w", "fused"):
        assert word in td, word
    for name in ('"mesh.tris"', '"mesh.verts"', '"mesh.bytes"', '"deform"'):  # the get_int names
        assert name in td and name in (PKG / "csrc" / "temporal.hip").read_text(), name
    sr = (ROOT / "include" / "srt_surface_refit.h").read_text()
    assert re.search(r"#define\s+SRT_SURFACE_REFIT_ABI_VERSION\s+1\b", sr) and re.search(r"#define\s+SRT_SURFACE_REFIT\s+1u", sr)
    assert _lib.SRT_SURFACE_REFIT == 1
    refit = (ROOT / "include" / "srt_refit.h").read_text()
    assert "need a re-created surface object" not in refit and "moved by `frame` only" not in refit  # the closed exclusions
    from srt_amd.surface import Surface
    from srt_amd.temporal import Temporal

    assert callable(Temporal.set_mesh) and callable(Temporal.set_vertices) and callable(Surface.refit)


def triangles(n):
    from srt_amd import _lib

    return (_lib.Triangle * n)()


def test_set_mesh_checks_before_any_device():
    """Counts, then the array, then the object; the message tells which check answered."""
    from srt_amd import _lib

    lib, inv, lim = _lib.lib(), _lib.SRT_ERR_INVALID, _lib.SRT_ERR_LIMIT
    tris = triangles(4)
    assert lib.srt_temporal_set_mesh(None, tris, 4, 9) == inv and "NULL object" in _lib.last_error()
    assert lib.srt_temporal_set_mesh(None, None, 0, 0) == inv and "NULL object" in _lib.last_error()  # a detach of nothing
    assert lib.srt_temporal_set_mesh(None, None, 4, 9) == inv and "NULL tris" in _lib.last_error()
    assert lib.srt_temporal_set_mesh(None, tris, 4, 0) == inv and "n_verts == 0" in _lib.last_error()
    for n_tris, n_verts in ((1 << 28, 9), (4, 1 << 28), (0xFFFFFFFF, 0xFFFFFFFF), (0, 1 << 28)):
        assert lib.srt_temporal_set_mesh(None, tris, n_tris, n_verts) == lim and "2^28" in _lib.last_error()
    assert lib.srt_temporal_set_mesh(None, None, 1 << 28, 0) == lim  # the limit before the array
    assert lib.srt_temporal_set_mesh(None, tris, (1 << 28) - 1, (1 << 28) - 1) == inv and "NULL object" in _lib.last_error()


def test_set_vertices_checks_before_any_device():
    from srt_amd import _lib

    lib, inv = _lib.lib(), _lib.SRT_ERR_INVALID
    buf = np.zeros(64, np.float32)
    base = buf.ctypes.data + (-buf.ctypes.data) % 16
    assert lib.srt_temporal_set_vertices(None, C.c_void_p(base), 2) == inv and "NULL object" in _lib.last_error()
    assert lib.srt_temporal_set_vertices(None, None, 0) == inv and "NULL object" in _lib.last_error()
    for off in (4, 8, 12):
        assert lib.srt_temporal_set_vertices(None, C.c_void_p(base + off), 2) == inv and "aligned" in _lib.last_error()


def test_surface_refit_checks_before_any_device():
    from srt_amd import _lib

    import surface_scenes as SS
    from srt_amd import _ptr

    lib, inv = _lib.lib(), _lib.SRT_ERR_INVALID
    assert lib.srt_surface_refit(None, None, 0) == inv
    s = SS.textured_scene()
    h = C.c_void_p()
    args = (_ptr(s.bvhs), len(s.bvhs), _ptr(s.mats), None, len(s.mats), _ptr(s.tris), len(s.tris), _ptr(s.verts), len(s.verts))
    assert lib.srt_surface_create_ex(0, None, *args, 2, C.byref(h)) == inv and "unknown flag" in _lib.last_error() and not h
    assert lib.srt_surface_create_ex(0, None, *args, 1, None) == inv
    bad = s.tris.copy()
    bad["v"][1, 2] = len(s.verts)  # srt_surface_create's validation, before the device, with the flag too
    args = args[:5] + (_ptr(bad),) + args[6:]
    assert lib.srt_surface_create_ex(0, None, *args, 1, C.byref(h)) == inv and "vertex index" in _lib.last_error()
    assert lib.srt_surface_create_obj_ex(0, None, None, 1, C.byref(h)) == inv


def test_cpp_mirrors_compile():
    """include/srt/temporal.hpp and include/srt/surface.hpp with the new members compile on their own (syntax only)."""
    src = ('#include "srt/temporal.hpp"\n#include "srt/surface.hpp"\n'
           "int use(srt::Temporal& t, srt::Surface& s, const srt_triangle* tris, const srt_vertex* verts_dev) {\n"
           "  t.SetMesh(tris, 32, 25); t.SetVertices(verts_dev, 25); t.SetVertices(nullptr, 25); t.SetMesh(nullptr, 0, 0);\n"
           "  s.Refit(verts_dev, 25);\n"
           '  return t.get_int("mesh.bytes") + t.get_int("deform") + s.get_int("refit") + SRT_TEMPORAL_DEFORM_ABI_VERSION\n'
           "         + SRT_SURFACE_REFIT_ABI_VERSION + (int)SRT_SURFACE_REFIT; }\n")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", str(ROOT / "include"), "-x", "c++", "-"],
                   input=src, text=True, check=True)


def test_mesh_bookkeeping_under_sanitizers():
    """tests/cpp/test_temporal_deform_host.cpp with csrc/temporal_host.cpp linked directly, AddressSanitizer + UBSan,
    as a stand-alone program (host code only: no HIP, no device, nothing preloaded): validation, which instance runs,
    the launch counts, V and V' over set_mesh / set_vertices / reset, and the deform records."""
    out = ROOT / "tests" / "cpp" / "_build"
    out.mkdir(exist_ok=True)
    exe = out / "test_temporal_deform_host_san"
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-Wall", "-ffp-contract=off", "-I", str(ROOT / "include"),
                    str(ROOT / "tests" / "cpp" / "test_temporal_deform_host.cpp"), str(PKG / "csrc" / "temporal_host.cpp"),
                    "-o", str(exe), "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-fno-omit-frame-pointer"], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "temporal deform host checks OK" in r.stdout
