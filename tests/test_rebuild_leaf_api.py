"""The leaf collapse of the device rebuild (include/srt_rebuild_leaf.h), CPU only: the host mirror
srt_bvh_build_lbvh_leaf against a numpy restatement of rules 4a-4c (tests/rebuild_leaf_ref.py) on every scene of
tests/rebuild_ref.py with max_leaf in {1, 2, 3, 4, 8, 255}; max_leaf == 1 against srt_bvh_build_lbvh byte for byte; the
order's independence of max_leaf; leaf and node sizes; the boxes against srt_bvh_refit; the oracle on the collapsed Rubik
tree; argument errors without a device; the exported symbols; the C++ mirror; and the host pieces under ASan/UBSan as a
stand-alone program."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import rebuild_leaf_ref as LR
import rebuild_ref as BR
import refit_ref as RR
import srt_amd as S
from conftest import OBJECTS, PKG, ROOT
from oracle import pyoracle as O
from srt_amd import _lib

MISS = 0xFFFFFFFF
NAMES = ["srt_rebuild_leaf_abi_version", "srt_query_set_rebuild_leaf", "srt_bvh_build_lbvh_leaf"]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def rubik():
    return S.load_obj(OBJECTS / "Rubik" / "Rubik.obj")


@pytest.fixture(scope="module")
def cases(rubik):
    """{name: (scene, verts, srt_bvh_build_lbvh's scene and order, {max_leaf: (host-built scene, order)})}."""
    out = {}
    for name in BR.SCENES:
        scene, verts = BR.make_scene(name, rubik)
        plain, order = S.build_lbvh(scene, verts)
        out[name] = (scene, verts, plain, order, {L: S.build_lbvh(scene, verts, max_leaf=L) for L in LR.LEAVES})
    return out


def test_library_exports_and_binding():
    text = (ROOT / "include" / "srt_rebuild_leaf.h").read_text()
    assert "#define SRT_REBUILD_LEAF_ABI_VERSION 1" in text
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = sorted(set(re.findall(r"\b(srt_[a-z0-9_]+)\s*\(", text)))
    assert names == sorted(NAMES) == sorted(_lib.REBUILD_LEAF_SYMBOLS)
    out = subprocess.run(["nm", "-D", "--defined-only", str(PKG / "libsrt_amd.so")], capture_output=True, text=True,
                         check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert not [n for n in names if n not in exported]
    lib = _lib.lib()
    assert lib.srt_rebuild_leaf_abi_version() == 1
    # the additive header leaves the others alone
    assert lib.srt_rebuild_abi_version() == 1 and lib.srt_refit_abi_version() == 1 and lib.srt_query_abi_version() == 1
    assert lib.srt_abi_version() == 2
    for n in names:
        assert isinstance(getattr(lib, n), C._CFuncPtr)
    # srt_rebuild.h's out-of-scope note points here
    assert "srt_rebuild_leaf.h" in (ROOT / "include" / "srt_rebuild.h").read_text()


@pytest.mark.parametrize("max_leaf", LR.LEAVES)
@pytest.mark.parametrize("name", BR.SCENES)
def test_children_leaves_and_numbering_equal_the_numpy_restatement(cases, name, max_leaf):
    scene, verts, plain, order, built = cases[name]
    tree, _ = built[max_leaf]
    k = BR.keys(scene, verts)[order]
    want_root, want_pairs = LR.collapsed(k, max_leaf)
    got_root, got_pairs = LR.host_tree(tree.nodes)
    assert got_root == want_root and got_pairs == want_pairs
    m = len(want_pairs)
    assert len(tree.nodes) == 2 * m + 1 and int(tree.bvhs[0]["first_index"]) == 0 and int(tree.bvhs[0]["count"]) == 2 * m + 1
    assert RR.reached(tree).all()
    n = len(scene.tris)
    if n <= max_leaf:
        assert m == 0 and want_root == ("leaf", 0, n)
    if name == "three" and max_leaf == 2:  # one 1-leaf and one 2-leaf
        assert sorted(int(c) for c in tree.nodes["count"]) == [0, 1, 2]
    if name == "copies" and max_leaf in (2, 4, 8):  # every key equal: the positions decide, a balanced tree
        assert m == 64 // max_leaf - 1 and set(tree.nodes["count"].tolist()) == {0, max_leaf}


@pytest.mark.parametrize("name", BR.SCENES)
def test_max_leaf_one_is_srt_bvh_build_lbvh_byte_for_byte(cases, name):
    scene, verts, plain, order, built = cases[name]
    n = len(scene.tris)
    nodes, tris, out = np.zeros(2 * n - 1, S.NODE_DTYPE), np.zeros(n, S.TRI_DTYPE), np.zeros(n, np.uint32)
    n_nodes = C.c_uint32(0)
    assert _lib.lib().srt_bvh_build_lbvh_leaf(S._ptr(scene.tris), n, S._ptr(verts), len(verts), 1, S._ptr(nodes), C.byref(n_nodes),
                                              S._ptr(tris), S._ptr(out)) == _lib.SRT_OK
    assert n_nodes.value == 2 * n - 1 == len(plain.nodes)
    assert nodes.tobytes() == plain.nodes.tobytes() and tris.tobytes() == plain.tris.tobytes()
    assert out.tobytes() == order.tobytes()
    one, order_one = built[1]  # the Python mirror's max_leaf=1 is the plain call
    assert one.nodes.tobytes() == plain.nodes.tobytes() and (order_one == order).all()


@pytest.mark.parametrize("name", BR.SCENES)
def test_order_and_triangles_do_not_depend_on_max_leaf(cases, name):
    scene, verts, plain, order, built = cases[name]
    for max_leaf, (tree, o) in built.items():
        assert o.tobytes() == order.tobytes(), max_leaf
        assert tree.tris.tobytes() == plain.tris.tobytes(), max_leaf
        assert (bits(tree.verts) == bits(verts)).all()


@pytest.mark.parametrize("max_leaf", LR.LEAVES)
@pytest.mark.parametrize("name", BR.SCENES)
def test_leaves_hold_at_most_max_leaf_and_internal_nodes_more(cases, name, max_leaf):
    scene, verts, plain, order, built = cases[name]
    nodes = built[max_leaf][0].nodes
    n = len(scene.tris)
    size = LR.leaf_sizes(nodes)
    leaf = nodes["count"] > 0
    assert (nodes["count"][leaf] <= max_leaf).all()
    assert (size[~leaf] > max_leaf).all()
    assert size[0] == n
    # every position in exactly one leaf
    covered = np.zeros(n, np.int64)
    for first, count in zip(nodes["first"][leaf], nodes["count"][leaf]):
        covered[int(first):int(first) + int(count)] += 1
    assert (covered == 1).all()
    m, largest, depth = LR.shape(nodes)
    m1, _, depth1 = LR.shape(plain.nodes)
    assert m <= m1 and depth <= depth1 and largest <= max_leaf  # depth and pairs only shrink


@pytest.mark.parametrize("max_leaf", LR.LEAVES)
@pytest.mark.parametrize("name", BR.SCENES)
def test_boxes_equal_the_host_refit_of_the_same_nodes(cases, name, max_leaf):
    scene, verts, plain, order, built = cases[name]
    tree = built[max_leaf][0]
    assert (bits(S.refit_scene(tree, verts).nodes) == bits(tree.nodes)).all()
    assert (bits(RR.refit_nodes(tree, verts)) == bits(tree.nodes)).all()
    blank = tree.nodes.copy()
    blank["min"], blank["max"] = 7.0, -7.0
    assert (bits(RR.refit_nodes(S.Scene(tree.bvhs, blank, tree.mats, tree.tex_albedo, tree.tris, tree.verts), verts))
            == bits(tree.nodes)).all()


@pytest.mark.parametrize("max_leaf", [2, 3, 4, 8, 255])
def test_the_oracle_reports_the_same_hits_on_the_collapsed_tree(cases, max_leaf):
    """Rays started outside the scene box: the collapsed tree and the max_leaf == 1 tree hold the same fp32 triangles at
    the same positions, so every closest distance agrees in its bits, and so does the creation-order triangle."""
    from test_gpu_queries import bounds, sphere_rays

    scene, verts, plain, order, built = cases["rubik"]
    tree, o = built[max_leaf]
    lo, hi = bounds(plain)
    rays = sphere_rays(lo, hi, 4099, 404)
    tri_1, t_1, _, st_1 = O.Oracle(plain).trace_closest(1, rays)
    tri_c, t_c, _, st_c = O.Oracle(tree).trace_closest(1, rays)
    assert st_1["stack_overflow"] == 0 and st_c["stack_overflow"] == 0
    hit = tri_1 != MISS
    assert hit.sum() >= 100 and 0.25 < hit.mean() < 0.95
    assert (hit == (tri_c != MISS)).all()
    assert (bits(t_1) == bits(t_c)).all()
    differ = order[tri_1[hit]] != o[tri_c[hit]]
    print(f"max_leaf {max_leaf}: {int(hit.sum())} hits, {int(differ.sum())} creation-order triangles differ")
    assert not differ.any()


def test_null_and_bad_arguments_without_a_device(cases):
    lib = _lib.lib()
    assert lib.srt_query_set_rebuild_leaf(None, 4) == _lib.SRT_ERR_INVALID and "null object" in _lib.last_error()
    assert lib.srt_query_set_rebuild_leaf(None, 0) == _lib.SRT_ERR_INVALID
    scene, verts, plain, order, built = cases["three"]
    nodes, tris, out = np.zeros(5, S.NODE_DTYPE), np.zeros(3, S.TRI_DTYPE), np.zeros(3, np.uint32)
    n_nodes = C.c_uint32(99)
    args = [S._ptr(scene.tris), 3, S._ptr(verts), len(verts), 2, S._ptr(nodes), C.byref(n_nodes), S._ptr(tris), S._ptr(out)]
    assert lib.srt_bvh_build_lbvh_leaf(*args) == _lib.SRT_OK and (out == order).all() and n_nodes.value == 3
    for k in (0, 2, 5, 6, 7, 8):
        bad = list(args)
        bad[k] = None
        assert lib.srt_bvh_build_lbvh_leaf(*bad) == _lib.SRT_ERR_INVALID
    bad = list(args)
    bad[1] = 0
    assert lib.srt_bvh_build_lbvh_leaf(*bad) == _lib.SRT_ERR_INVALID and "at least one triangle" in _lib.last_error()
    for max_leaf in (0, 256, 0xFFFFFFFF):  # the outputs stay as they were
        bad = list(args)
        bad[4] = max_leaf
        out[:] = 77
        n_nodes.value = 99
        assert lib.srt_bvh_build_lbvh_leaf(*bad) == _lib.SRT_ERR_INVALID and "[1, 255]" in _lib.last_error()
        assert (out == 77).all() and n_nodes.value == 99
        with pytest.raises(S.SrtError):
            S.build_lbvh(scene, verts, max_leaf=max_leaf)
    for value in (np.inf, -np.inf, np.nan):  # a vertex the host can check and the device cannot
        v = verts.copy()
        v[1]["pos"][2] = value
        out[:] = 77
        bad = list(args)
        bad[2] = S._ptr(v)
        assert lib.srt_bvh_build_lbvh_leaf(*bad) == _lib.SRT_ERR_INVALID
        assert "not finite" in _lib.last_error() and (out == 77).all()


def test_python_argument_checks_without_a_device(rubik, cases):
    from srt_amd.query import Query

    scene = cases["rubik"][0]
    with pytest.raises(ValueError, match="needs rebuild=True"):
        Query(scene, refit=True, rebuild_leaf=4)
    with pytest.raises(ValueError, match="needs refit=True"):
        Query(scene, rebuild=True, rebuild_leaf=4)
    two = S.Scene.from_models([rubik, S.model_from_triangles(RR.grid_triangles(2))])
    with pytest.raises(ValueError, match="one model"):
        S.build_lbvh(two, max_leaf=4)
    built, order = S.build_lbvh(scene, max_leaf=4)  # the scene's own vertices
    assert (bits(built.verts) == bits(scene.verts)).all() and (scene.tri_input[order] == built.tri_input).all()


def test_rebuild_leaf_host_under_sanitizers():
    """tests/cpp/test_rebuild_leaf_host.cpp with csrc/rebuild_host.cpp and csrc/refit_host.cpp alone, AddressSanitizer +
    UBSan, as a stand-alone program with its own main (host code only: no HIP, no device, nothing preloaded): the
    package's `make SAN=1 test_rebuild_leaf_host` builds and runs it."""
    r = subprocess.run(["make", "-s", "-C", str(PKG), "SAN=1", "test_rebuild_leaf_host"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "rebuild leaf host checks OK" in r.stdout
    exe = PKG / "build_san" / "test_rebuild_leaf_host"
    out = subprocess.run(["nm", str(exe)], capture_output=True, text=True, check=True).stdout
    assert "__asan_init" in out and "__ubsan_handle" in out  # the program is instrumented
    assert "hipMalloc" not in out and "BuildLayout" not in out  # host pieces only: no HIP, no query_host.cpp


def test_cpp_mirror_compiles_and_builds_on_the_host():
    """include/srt/query.hpp: Query::SetRebuildLeaf and the AssetUtils::BuildLBVH overload against the C ABI."""
    out = ROOT / "tests" / "cpp" / "_build"
    out.mkdir(exist_ok=True)
    exe = out / "test_rebuild_leaf_mirror"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", str(ROOT / "include"),
                    str(ROOT / "tests" / "cpp" / "test_rebuild_leaf_mirror.cpp"), "-o", str(exe), "-L", str(PKG), "-lsrt_amd",
                    f"-Wl,-rpath,{PKG}"], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "rebuild leaf mirror OK" in r.stdout, r.stdout + r.stderr
