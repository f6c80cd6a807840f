"""The ray-query service's boundary (include/srt_query.h), CPU only: exported symbols, record layout, argument
and scene validation before any device is touched, the host-side re-layout under ASan/UBSan as a stand-alone
program, and the identity of the path tracer's device code (the new translation unit must not move it)."""
import ctypes as C
import json
import re
import subprocess

import numpy as np

from conftest import OBJECTS, PKG, ROOT


def declared_functions():
    text = (ROOT / "include" / "srt_query.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(srt_query_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_query_symbol():
    names = declared_functions()
    for n in ("srt_query_abi_version", "srt_query_create", "srt_query_create_obj", "srt_query_destroy",
              "srt_query_set_bvh_count", "srt_query_update_model_matrix", "srt_query_closest", "srt_query_occluded",
              "srt_query_get_int"):
        assert n in names
    out = subprocess.run(["nm", "-D", "--defined-only", str(PKG / "libsrt_amd.so")], capture_output=True, text=True,
                         check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert not [n for n in names if n not in exported]


def test_python_binding_and_versions():
    from srt_amd import _lib

    assert set(declared_functions()) == set(_lib.QUERY_SYMBOLS)
    lib = _lib.lib()
    assert lib.srt_query_abi_version() == 1
    assert lib.srt_abi_version() == 2  # the additive entry points leave srt_amd.h's version alone
    for n in declared_functions():
        assert isinstance(getattr(lib, n), C._CFuncPtr)


def test_hit_record_layout():
    from srt_amd import _lib
    from srt_amd.query import HIT_DTYPE

    assert C.sizeof(_lib.Hit) == 32
    offs = {n: getattr(_lib.Hit, n).offset for n, _ in _lib.Hit._fields_}
    assert (offs["triangle"], offs["t"], offs["normal"], offs["material"], offs["bvh"]) == (0, 4, 8, 20, 24)
    assert HIT_DTYPE.itemsize == 32
    assert [HIT_DTYPE.fields[n][1] for n in ("triangle", "t", "normal", "material", "bvh")] == [0, 4, 8, 20, 24]


def test_code_hash_is_the_one_the_counters_were_taken_on():
    """`make -s hash` (the preprocessed pathtrace.hip translation unit and the hipcc flags) still equals every
    code_hash stamped into profiles/counters.json: the query service lives in its own translation unit."""
    h = subprocess.run(["make", "-s", "-C", str(PKG), "hash"], capture_output=True, text=True, check=True).stdout.strip()
    assert re.fullmatch(r"[0-9a-f]{16}", h)
    text = (ROOT / "profiles" / "counters.json").read_text()
    stamped = set(re.findall(r'"code_hash"\s*:\s*"([0-9a-f]+)"', text))
    assert stamped == {h}, (stamped, h)
    json.loads(text)


def test_null_and_bad_arguments():
    from srt_amd import _lib

    lib = _lib.lib()
    assert lib.srt_query_closest(None, None, 4, None) == _lib.SRT_ERR_INVALID
    assert lib.srt_query_occluded(None, None, 4, None) == _lib.SRT_ERR_INVALID
    assert lib.srt_query_destroy(None) == _lib.SRT_ERR_INVALID
    assert lib.srt_query_set_bvh_count(None, 1) == _lib.SRT_ERR_INVALID
    assert lib.srt_query_update_model_matrix(None, 0, None) == _lib.SRT_ERR_INVALID
    v = C.c_int()
    assert lib.srt_query_get_int(None, b"stack.entries", C.byref(v)) == _lib.SRT_ERR_INVALID
    assert lib.srt_query_create_obj(0, None, None, None) == _lib.SRT_ERR_INVALID


def test_create_validates_the_scene_before_touching_a_device():
    """A child index >= n_nodes, a triangle range past n_tris and a root past n_nodes are rejected on the host
    (this machine may have no GPU: a call that reached the device would fail with SRT_ERR_HIP instead)."""
    import srt_amd as S
    from srt_amd import _lib

    lib = _lib.lib()
    scene = S.Scene.from_models([S.load_obj(OBJECTS / "Rubik" / "Rubik.obj")])

    def create(bvhs, nodes, tris):
        h = C.c_void_p()
        rc = lib.srt_query_create(0, None, S._ptr(bvhs), len(bvhs), S._ptr(nodes), len(nodes), S._ptr(tris), len(tris),
                                  S._ptr(scene.verts), len(scene.verts), C.byref(h))
        assert h.value is None or rc == _lib.SRT_OK
        return rc

    internal = int(np.flatnonzero(scene.nodes["count"] == 0)[3])
    leaf = int(np.flatnonzero(scene.nodes["count"] > 0)[5])
    nodes = scene.nodes.copy()
    nodes[internal]["first"] = len(nodes)
    assert create(scene.bvhs, nodes, scene.tris) == _lib.SRT_ERR_INVALID
    assert "children out of range" in _lib.last_error()
    nodes = scene.nodes.copy()
    nodes[internal]["first"] = len(nodes) - 1  # the second child is one past the array
    assert create(scene.bvhs, nodes, scene.tris) == _lib.SRT_ERR_INVALID
    nodes = scene.nodes.copy()
    nodes[leaf]["first"] = len(scene.tris)
    assert create(scene.bvhs, nodes, scene.tris) == _lib.SRT_ERR_INVALID
    assert "triangles out of range" in _lib.last_error()
    nodes = scene.nodes.copy()
    nodes[leaf]["count"] = 0x80000000
    assert create(scene.bvhs, nodes, scene.tris) == _lib.SRT_ERR_INVALID
    bvhs = scene.bvhs.copy()
    bvhs[0]["first_index"] = len(scene.nodes)
    assert create(bvhs, scene.nodes, scene.tris) == _lib.SRT_ERR_INVALID
    assert create(scene.bvhs, scene.nodes, scene.tris[:0]) == _lib.SRT_ERR_INVALID  # n_tris = 0
    assert create(scene.bvhs[:0], scene.nodes, scene.tris) == _lib.SRT_ERR_INVALID


def _build_host_program(name, extra):
    out = ROOT / "tests" / "cpp" / "_build"
    out.mkdir(exist_ok=True)
    exe = out / name
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-Wall", "-I", str(ROOT / "include"),
                    str(ROOT / "tests" / "cpp" / "test_query_host.cpp"), str(PKG / "csrc" / "query_host.cpp"),
                    "-o", str(exe), *extra], check=True)
    return exe


def test_host_relayout_under_sanitizers():
    """tests/cpp/test_query_host.cpp with csrc/query_host.cpp linked directly, AddressSanitizer + UBSan, as a
    stand-alone program (host code only: no HIP, no device, nothing preloaded)."""
    exe = _build_host_program("test_query_host_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                                                      "-fno-omit-frame-pointer"])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "query host checks OK" in r.stdout


def test_host_relayout_of_rubik():
    """The same program against the library's loader (no sanitizer): Rubik's arrays re-laid."""
    exe = _build_host_program("test_query_host", ["-DWITH_LIBSRT", "-L", str(PKG), "-lsrt_amd", f"-Wl,-rpath,{PKG}"])
    r = subprocess.run([str(exe), str(OBJECTS / "Rubik" / "Rubik.obj")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Rubik: 1188 triangles" in r.stdout and "query host checks OK" in r.stdout
