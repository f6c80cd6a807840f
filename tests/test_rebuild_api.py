"""The device rebuild's boundary (include/srt_rebuild.h), CPU only: exported symbols, the host mirror srt_bvh_build_lbvh
against a numpy restatement of its rule (tests/rebuild_ref.py) -- keys, order and hierarchy -- the tree's shape and boxes,
the oracle on the built tree, the host pieces under ASan/UBSan as a stand-alone program, the C++ mirror, and argument
errors without a device."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import rebuild_ref as BR
import refit_ref as RR
import srt_amd as S
from conftest import OBJECTS, PKG, ROOT
from oracle import pyoracle as O
from srt_amd import _lib

MISS = 0xFFFFFFFF
NAMES = ["srt_rebuild_abi_version", "srt_query_enable_rebuild", "srt_query_rebuild", "srt_query_tri_order",
         "srt_bvh_build_lbvh"]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def rubik():
    return S.load_obj(OBJECTS / "Rubik" / "Rubik.obj")


@pytest.fixture(scope="module")
def cases(rubik):
    """{name: (scene, verts, host-built scene, order)}."""
    out = {}
    for name in BR.SCENES:
        scene, verts = BR.make_scene(name, rubik)
        built, order = S.build_lbvh(scene, verts)
        out[name] = (scene, verts, built, order)
    return out


def test_library_exports_and_binding():
    text = (ROOT / "include" / "srt_rebuild.h").read_text()
    assert "#define SRT_REBUILD_ABI_VERSION 1" in text
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = sorted(set(re.findall(r"\b(srt_[a-z0-9_]+)\s*\(", text)))
    assert names == sorted(NAMES) == sorted(_lib.REBUILD_SYMBOLS)
    out = subprocess.run(["nm", "-D", "--defined-only", str(PKG / "libsrt_amd.so")], capture_output=True, text=True,
                         check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert not [n for n in names if n not in exported]
    lib = _lib.lib()
    assert lib.srt_rebuild_abi_version() == 1
    # the additive header leaves the others alone
    assert lib.srt_refit_abi_version() == 1 and lib.srt_query_abi_version() == 1 and lib.srt_abi_version() == 2
    for n in names:
        assert isinstance(getattr(lib, n), C._CFuncPtr)


@pytest.mark.parametrize("name", BR.SCENES)
def test_keys_order_and_hierarchy_equal_the_numpy_restatement(cases, name):
    scene, verts, built, order = cases[name]
    n = len(scene.tris)
    k = BR.keys(scene, verts)
    assert (order == BR.order(k)).all()
    assert sorted(order.tolist()) == list(range(n))  # a permutation
    assert (bits(built.tris) == bits(scene.tris[order])).all()
    assert (bits(built.verts) == bits(verts)).all()
    assert len(built.nodes) == 2 * n - 1 and int(built.bvhs[0]["first_index"]) == 0
    assert BR.host_children(built.nodes) == BR.hierarchy(k[order])
    # every leaf holds one triangle, every triangle one leaf
    leaves = built.nodes[built.nodes["count"] > 0]
    assert (leaves["count"] == 1).all() and sorted(leaves["first"].tolist()) == list(range(n))
    assert RR.reached(built).all()
    if name == "grid_flat":
        lo, hi = BR.scene_box(scene, verts)
        assert lo[2] == hi[2] and (k & 0x09249249 == 0).all()  # no extent in z: its bits are all zero
    elif name == "grid":
        assert n == 1152 and RR.pair_height_counts(built)[0] > 256  # (a per-level launch and the fused tail both run)
    elif name == "copies":
        assert n == 64 and len(set(k.tolist())) == 1 and (order == np.arange(n)).all()
        assert len(RR.pair_height_counts(built)) == 6  # balanced over the positions
    elif name == "oob":
        assert (scene.tris["v"] >= len(verts)).sum() == 2
        assert (BR.scene_box(scene, verts)[0] == 0).all() and verts["pos"].min() > 1
    elif name == "one":
        assert len(built.nodes) == 1 and built.nodes[0]["count"] == 1
    elif name == "two":
        assert (built.nodes["count"] == (0, 1, 1)).all() and (built.nodes["first"] == (1, 0, 1)).all()
    # the depth bound of the header: 30 + ceil(log2 n), and inside the oracle's 64-entry stack
    depth = len(RR.pair_height_counts(built)) if n > 1 else 0
    assert depth <= 30 + int(np.ceil(np.log2(n))) and depth + 1 <= 64


@pytest.mark.parametrize("name", BR.SCENES)
def test_boxes_equal_the_host_refit_of_the_same_nodes(cases, name):
    scene, verts, built, order = cases[name]
    assert (bits(S.refit_scene(built, verts).nodes) == bits(built.nodes)).all()  # (srt_bvh_refit validates as create does)
    assert (bits(RR.refit_nodes(built, verts)) == bits(built.nodes)).all()
    blank = built.nodes.copy()
    blank["min"], blank["max"] = 7.0, -7.0
    assert (bits(RR.refit_nodes(S.Scene(built.bvhs, blank, built.mats, built.tex_albedo, built.tris, built.verts), verts))
            == bits(built.nodes)).all()


def test_the_oracle_reports_the_same_distances_on_the_built_tree(cases):
    """Rays started outside the scene box: the LBVH and the scene's own midpoint tree, refit to the same vertices, test
    the same fp32 triangles, so every closest distance agrees in its bits (ids may differ where distances tie)."""
    from test_gpu_queries import bounds, sphere_rays

    scene, verts, built, order = cases["rubik"]
    refit = S.refit_scene(scene, verts)
    lo, hi = bounds(refit)
    rays = sphere_rays(lo, hi, 4099, 404)
    tri_r, t_r, _, st_r = O.Oracle(refit).trace_closest(1, rays)
    tri_b, t_b, _, st_b = O.Oracle(built).trace_closest(1, rays)
    assert st_r["stack_overflow"] == 0 and st_b["stack_overflow"] == 0
    hit = tri_r != MISS
    assert 0.25 < hit.mean() < 0.95
    assert (hit == (tri_b != MISS)).all()
    assert (bits(t_r) == bits(t_b)).all()
    assert (order[tri_b[hit]] == tri_r[hit]).mean() > 0.99


def test_rebuild_host_under_sanitizers():
    """tests/cpp/test_rebuild_host.cpp with csrc/rebuild_host.cpp, csrc/refit_host.cpp and csrc/query_host.cpp linked
    directly, AddressSanitizer + UBSan, as a stand-alone program (host code only: no HIP, no device, nothing preloaded)."""
    out = ROOT / "tests" / "cpp" / "_build"
    out.mkdir(exist_ok=True)
    exe = out / "test_rebuild_host_san"
    src = [str(PKG / "csrc" / f) for f in ("rebuild_host.cpp", "refit_host.cpp", "query_host.cpp")]
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-Wall", "-ffp-contract=off", "-I", str(ROOT / "include"),
                    str(ROOT / "tests" / "cpp" / "test_rebuild_host.cpp"), *src, "-o", str(exe),
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "rebuild host checks OK" in r.stdout


def test_cpp_mirror_compiles_and_builds_on_the_host():
    """include/srt/query.hpp: Query::EnableRebuild, Query::Rebuild and AssetUtils::BuildLBVH against the C ABI."""
    out = ROOT / "tests" / "cpp" / "_build"
    out.mkdir(exist_ok=True)
    exe = out / "test_rebuild_mirror"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", str(ROOT / "include"), str(ROOT / "tests" / "cpp" / "test_rebuild_mirror.cpp"),
                    "-o", str(exe), "-L", str(PKG), "-lsrt_amd", f"-Wl,-rpath,{PKG}"], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "rebuild mirror OK" in r.stdout, r.stdout + r.stderr


def test_null_and_bad_arguments_without_a_device(cases):
    lib = _lib.lib()
    buf = (C.c_uint8 * 64)()
    assert lib.srt_query_enable_rebuild(None) == _lib.SRT_ERR_INVALID and "null object" in _lib.last_error()
    assert lib.srt_query_rebuild(None, buf, 2) == _lib.SRT_ERR_INVALID and "null object" in _lib.last_error()
    assert lib.srt_query_rebuild(None, None, 0) == _lib.SRT_ERR_INVALID
    assert lib.srt_query_tri_order(None, buf, 2) == _lib.SRT_ERR_INVALID
    scene, verts, built, order = cases["three"]
    nodes, tris, out = np.zeros(5, S.NODE_DTYPE), np.zeros(3, S.TRI_DTYPE), np.zeros(3, np.uint32)
    args = [S._ptr(scene.tris), 3, S._ptr(verts), len(verts), S._ptr(nodes), S._ptr(tris), S._ptr(out)]
    assert lib.srt_bvh_build_lbvh(*args) == _lib.SRT_OK and (out == order).all()
    for k in (0, 2, 4, 5, 6):
        bad = list(args)
        bad[k] = None
        assert lib.srt_bvh_build_lbvh(*bad) == _lib.SRT_ERR_INVALID
    bad = list(args)
    bad[1] = 0
    assert lib.srt_bvh_build_lbvh(*bad) == _lib.SRT_ERR_INVALID and "at least one triangle" in _lib.last_error()
    # a vertex the host can check and the device cannot; the outputs stay as they were
    for value in (np.inf, -np.inf, np.nan):
        v = verts.copy()
        v[1]["pos"][2] = value
        out[:] = 77
        assert lib.srt_bvh_build_lbvh(S._ptr(scene.tris), 3, S._ptr(v), len(v), S._ptr(nodes), S._ptr(tris),
                                      S._ptr(out)) == _lib.SRT_ERR_INVALID
        assert "not finite" in _lib.last_error() and (out == 77).all()
        with pytest.raises(S.SrtError):
            S.build_lbvh(scene, v)


def test_python_argument_checks_without_a_device(rubik, cases):
    from srt_amd.query import Query

    scene = cases["rubik"][0]
    with pytest.raises(ValueError, match="needs refit=True"):
        Query(scene, rebuild=True)
    two = S.Scene.from_models([rubik, S.model_from_triangles(RR.grid_triangles(2))])
    with pytest.raises(ValueError, match="one model"):
        S.build_lbvh(two)
    built, order = S.build_lbvh(scene)  # the scene's own vertices
    assert (bits(built.verts) == bits(scene.verts)).all() and (scene.tri_input[order] == built.tri_input).all()
