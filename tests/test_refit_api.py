"""The BVH refit's boundary (include/srt_refit.h), CPU only: exported symbols, the host refit srt_bvh_refit against a
numpy restatement of its rule (tests/refit_ref.py) bit for bit, the identity refit, conservativeness by the oracle
alone, validation, the host pieces under ASan/UBSan as a stand-alone program, and argument errors without a device."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import refit_ref as RR
import srt_amd as S
from conftest import OBJECTS, PKG, ROOT
from oracle import pyoracle as O
from srt_amd import _lib

MISS = 0xFFFFFFFF


def declared_functions():
    text = (ROOT / "include" / "srt_refit.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(srt_[a-z0-9_]+)\s*\(", text)))


@pytest.fixture(scope="module")
def rubik():
    return S.load_obj(OBJECTS / "Rubik" / "Rubik.obj")


@pytest.fixture(scope="module")
def scenes(rubik):
    grid = S.model_from_triangles(RR.grid_triangles())
    return {"rubik": S.Scene.from_models([rubik]), "grid": S.Scene.from_models([grid]),
            "two": S.Scene.from_models([rubik, grid])}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def host_refit(scene, nodes, verts, bvhs=None, tris=None):
    bvhs = scene.bvhs if bvhs is None else bvhs
    tris = scene.tris if tris is None else tris
    return _lib.lib().srt_bvh_refit(S._ptr(bvhs), len(bvhs), S._ptr(nodes), len(nodes), S._ptr(tris), len(tris),
                                    S._ptr(verts), len(verts))


def test_library_exports_and_binding():
    names = declared_functions()
    assert names == sorted(["srt_refit_abi_version", "srt_bvh_refit", "srt_query_create_ex", "srt_query_create_obj_ex",
                            "srt_query_refit", "srt_query_copy_layout"])
    assert set(names) == set(_lib.REFIT_SYMBOLS)
    out = subprocess.run(["nm", "-D", "--defined-only", str(PKG / "libsrt_amd.so")], capture_output=True, text=True,
                         check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert not [n for n in names if n not in exported]
    lib = _lib.lib()
    assert lib.srt_refit_abi_version() == 1
    assert lib.srt_query_abi_version() == 1 and lib.srt_abi_version() == 2  # the additive header leaves both alone
    for n in names:
        assert isinstance(getattr(lib, n), C._CFuncPtr)


@pytest.mark.parametrize("name", ["rubik", "grid", "two"])
def test_host_refit_equals_the_numpy_restatement(scenes, name):
    scene = scenes[name]
    assert len(scene.bvhs) == (2 if name == "two" else 1)
    if name == "grid":
        assert len(scene.tris) == 1152
        assert RR.pair_height_counts(scene)[0] > 256  # (what the GPU test's per-level launch rests on)
    for amplitude, phase in ((RR.WAVE_AMPLITUDE, 0.0), (1.5, 0.7)):
        verts = RR.wave(scene.verts, amplitude, phase)
        want = RR.refit_nodes(scene, verts)
        got = S.refit_scene(scene, verts)
        assert (bits(got.nodes) == bits(want)).all()
        assert (bits(got.verts) == bits(verts)).all()
        assert not (bits(want) == bits(scene.nodes)).all()  # the restatement alone: the boxes moved
        # positions alone keep the scene's uvs
        assert (bits(S.refit_scene(scene, verts["pos"]).nodes) == bits(want)).all()
    assert (bits(scene.nodes) != bits(want)).any()  # refit_scene copies: the scene is as it was


@pytest.mark.parametrize("name", ["rubik", "grid", "two"])
def test_identity_refit_reproduces_the_builder(scenes, name):
    scene = scenes[name]
    assert RR.reached(scene).all()  # the builder leaves no orphan: the comparison below covers every node
    got = S.refit_scene(scene, scene.verts).nodes
    assert (got["min"] == scene.nodes["min"]).all() and (got["max"] == scene.nodes["max"]).all()  # (-0 == +0)
    assert (got["first"] == scene.nodes["first"]).all() and (got["count"] == scene.nodes["count"]).all()
    # nodes no traversal reaches are untouched, whatever they hold
    nodes = np.concatenate([scene.nodes, scene.nodes[:3]])
    nodes[-3:]["min"], nodes[-3:]["max"] = np.nan, -7.0
    nodes[-3:]["first"], nodes[-3:]["count"] = 0xDEADBEEF, (0, 5, 0x80000000)
    before = nodes.copy()
    assert host_refit(scene, nodes, RR.wave(scene.verts)) == _lib.SRT_OK
    assert (bits(nodes[-3:]) == bits(before[-3:])).all()
    assert (bits(nodes[:-3]) == bits(RR.refit_nodes(scene, RR.wave(scene.verts)))).all()


def test_refit_boxes_are_conservative_by_the_oracle(scenes):
    """The refit tree and a tree rebuilt from the deformed triangles test the same fp32 triangles, so the closest
    distance of every ray agrees in its bits; only the boxes differ.  (Triangle ids are not compared: ties resolve
    by order.)"""
    from test_gpu_queries import bounds, sphere_rays

    scene = scenes["rubik"]
    verts = RR.wave(scene.verts)
    refit = S.refit_scene(scene, verts)
    lo, hi = bounds(refit)
    rays = sphere_rays(lo, hi, 4099, 404)
    tri_r, t_r, _, st_r = O.Oracle(refit).trace_closest(1, rays)
    tri_b, t_b, _, st_b = O.Oracle(RR.rebuilt_scene(scene, verts)).trace_closest(1, rays)
    assert st_r["stack_overflow"] == 0 and st_b["stack_overflow"] == 0
    hit = tri_r != MISS
    assert 0.25 < hit.mean() < 0.95
    assert (hit == (tri_b != MISS)).all()
    assert (bits(t_r) == bits(t_b)).all()


def test_validation_failures_leave_the_nodes_alone(scenes):
    scene = scenes["rubik"]
    lib = _lib.lib()
    verts = RR.wave(scene.verts)
    internal = int(np.flatnonzero(scene.nodes["count"] == 0)[3])
    leaf = int(np.flatnonzero(scene.nodes["count"] > 0)[5])

    def create_error(bvhs, nodes, tris):
        """srt_query_create's answer for the same arrays (host validation comes before any device)."""
        h = C.c_void_p()
        rc = lib.srt_query_create(0, None, S._ptr(bvhs), len(bvhs), S._ptr(nodes), len(nodes), S._ptr(tris), len(tris),
                                  S._ptr(verts), len(verts), C.byref(h))
        return rc, _lib.last_error()

    def rejected(nodes=None, bvhs=None, tris=None, v=None, same_as_create=True):
        nodes = scene.nodes.copy() if nodes is None else nodes
        bvhs = scene.bvhs if bvhs is None else bvhs
        tris = scene.tris if tris is None else tris
        before = nodes.copy()
        rc = host_refit(scene, nodes, verts if v is None else v, bvhs=bvhs, tris=tris)
        err = _lib.last_error()
        assert rc == _lib.SRT_ERR_INVALID and err
        assert (bits(nodes) == bits(before)).all()
        if same_as_create:
            assert create_error(bvhs, before, tris) == (rc, err)
        return err

    nodes = scene.nodes.copy()
    nodes[internal]["first"] = len(nodes)
    assert "children out of range" in rejected(nodes)
    nodes = scene.nodes.copy()
    nodes[internal]["first"] = len(nodes) - 1  # the second child is one past the array
    rejected(nodes)
    nodes = scene.nodes.copy()
    nodes[internal]["first"] = 0xFFFFFFFF
    rejected(nodes)
    nodes = scene.nodes.copy()
    nodes[leaf]["first"], nodes[leaf]["count"] = 0, 0  # a cycle back to the root
    assert "cycle" in rejected(nodes)
    nodes = scene.nodes.copy()
    nodes[leaf]["first"] = len(scene.tris)
    assert "triangles out of range" in rejected(nodes)
    nodes = scene.nodes.copy()
    nodes[leaf]["first"], nodes[leaf]["count"] = 0xFFFFFFFF, 2  # first + count wraps in 32 bits
    rejected(nodes)
    nodes = scene.nodes.copy()
    nodes[leaf]["count"] = 0x80000000
    rejected(nodes)
    bvhs = scene.bvhs.copy()
    bvhs[0]["first_index"] = len(scene.nodes)
    assert "first_index out of range" in rejected(bvhs=bvhs)
    rejected(tris=scene.tris[:0])   # n_tris = 0
    assert "at least one BVH" in rejected(bvhs=scene.bvhs[:0])
    nodes = scene.nodes.copy()
    assert lib.srt_bvh_refit(None, 1, S._ptr(nodes), len(nodes), S._ptr(scene.tris), len(scene.tris), S._ptr(verts),
                             len(verts)) == _lib.SRT_ERR_INVALID
    assert lib.srt_bvh_refit(S._ptr(scene.bvhs), 1, None, len(nodes), S._ptr(scene.tris), len(scene.tris), S._ptr(verts),
                             len(verts)) == _lib.SRT_ERR_INVALID
    # a vertex the host can check and the device cannot
    for bad in (np.inf, -np.inf, np.nan):
        for k in range(3):
            v = verts.copy()
            v[len(v) // 2]["pos"][k] = bad
            assert "not finite" in rejected(v=v, same_as_create=False)
            with pytest.raises(S.SrtError):
                S.refit_scene(scene, v)
    # and the good arrays still pass
    nodes = scene.nodes.copy()
    assert host_refit(scene, nodes, verts) == _lib.SRT_OK


def test_refit_host_under_sanitizers():
    """tests/cpp/test_refit_host.cpp with csrc/refit_host.cpp linked directly, AddressSanitizer + UBSan, as a
    stand-alone program (host code only: no HIP, no device, nothing preloaded): the schedule builder on hand-made
    trees, the leaf fold, the node refit and its validation."""
    out = ROOT / "tests" / "cpp" / "_build"
    out.mkdir(exist_ok=True)
    exe = out / "test_refit_host_san"
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-Wall", "-I", str(ROOT / "include"),
                    str(ROOT / "tests" / "cpp" / "test_refit_host.cpp"), str(PKG / "csrc" / "refit_host.cpp"), "-o", str(exe),
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "refit host checks OK" in r.stdout


def test_cpp_mirror_compiles_and_refits_on_the_host():
    """include/srt/query.hpp: the flags argument, Query::Refit and AssetUtils::RefitBVH against the C ABI."""
    out = ROOT / "tests" / "cpp" / "_build"
    out.mkdir(exist_ok=True)
    exe = out / "test_refit_mirror"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", str(ROOT / "include"), str(ROOT / "tests" / "cpp" / "test_refit_mirror.cpp"),
                    "-o", str(exe), "-L", str(PKG), "-lsrt_amd", f"-Wl,-rpath,{PKG}"], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "refit mirror OK" in r.stdout, r.stdout + r.stderr


def test_null_and_bad_arguments_without_a_device():
    lib = _lib.lib()
    buf = (C.c_uint8 * 64)()
    assert lib.srt_query_refit(None, None, 0) == _lib.SRT_ERR_INVALID
    assert lib.srt_query_refit(None, buf, 2) == _lib.SRT_ERR_INVALID
    assert lib.srt_query_copy_layout(None, None, None, None) == _lib.SRT_ERR_INVALID
    assert lib.srt_query_copy_layout(None, buf, buf, buf) == _lib.SRT_ERR_INVALID
    h = C.c_void_p()
    assert lib.srt_query_create_obj_ex(0, None, None, _lib.SRT_QUERY_REFIT, C.byref(h)) == _lib.SRT_ERR_INVALID
    assert lib.srt_query_create_ex(0, None, None, 0, None, 0, None, 0, None, 0, _lib.SRT_QUERY_REFIT, None) == _lib.SRT_ERR_INVALID
    assert lib.srt_bvh_refit(None, 0, None, 0, None, 0, None, 0) == _lib.SRT_ERR_INVALID


def test_unknown_flags_and_bad_scenes_are_rejected_before_a_device(scenes):
    scene = scenes["rubik"]
    lib = _lib.lib()

    def create(flags, nodes):
        h = C.c_void_p()
        rc = lib.srt_query_create_ex(0, None, S._ptr(scene.bvhs), len(scene.bvhs), S._ptr(nodes), len(nodes), S._ptr(scene.tris),
                                     len(scene.tris), S._ptr(scene.verts), len(scene.verts), flags, C.byref(h))
        assert h.value is None
        return rc

    assert create(2, scene.nodes) == _lib.SRT_ERR_INVALID and "unknown flags" in _lib.last_error()
    nodes = scene.nodes.copy()
    nodes[int(np.flatnonzero(nodes["count"] == 0)[3])]["first"] = len(nodes)
    assert create(_lib.SRT_QUERY_REFIT, nodes) == _lib.SRT_ERR_INVALID and "children out of range" in _lib.last_error()
