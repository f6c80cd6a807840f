"""The device rebuild for scenes of several models (include/srt_rebuild_models.h), CPU only: the host mirror
srt_bvh_build_lbvh_models against the single-model mirror run on every record alone and against a numpy restatement of the
segmented rule (tests/rebuild_models_ref.py), with max_leaf 1 and 4, up to 300 records and with the records' triangles interleaved; a one-record scene against srt_bvh_build_lbvh_leaf
byte for byte; the oracle on the mirror's arrays against the oracle on the host-refit scene; the refusals with their
messages; the exported symbols; the C++ mirror; and the host pieces under ASan/UBSan as a stand-alone program."""
import ctypes as C
import dataclasses
import re
import subprocess

import numpy as np
import pytest

import rebuild_leaf_ref as LR
import rebuild_models_ref as MR
import refit_ref as RR
import srt_amd as S
from conftest import OBJECTS, PKG, ROOT, bits_equal
from oracle import pyoracle as O
from srt_amd import _lib

MISS = 0xFFFFFFFF
NAMES = ["srt_rebuild_models_abi_version", "srt_query_enable_rebuild_models", "srt_bvh_build_lbvh_models"]
ALL = MR.SCENES + MR.EXTRA + MR.MANY + MR.MANY_MIXED


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def rubik():
    return S.load_obj(OBJECTS / "Rubik" / "Rubik.obj")


@pytest.fixture(scope="module")
def cases(rubik):
    """{name: (scene, verts, {max_leaf: (mirror-built scene, order)})}, once."""
    out = {}
    for name in ALL:
        scene, verts = MR.make_scene(name, rubik)
        out[name] = (scene, verts, {L: S.build_lbvh_models(scene, verts, max_leaf=L) for L in MR.LEAVES})
    return out


def test_library_exports_and_binding():
    text = (ROOT / "include" / "srt_rebuild_models.h").read_text()
    assert "#define SRT_REBUILD_MODELS_ABI_VERSION 1" in text
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = sorted(set(re.findall(r"\b(srt_[a-z0-9_]+)\s*\(", text)))
    assert names == sorted(NAMES) == sorted(_lib.REBUILD_MODELS_SYMBOLS)
    out = subprocess.run(["nm", "-D", "--defined-only", str(PKG / "libsrt_amd.so")], capture_output=True, text=True,
                         check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert not [n for n in names if n not in exported]
    lib = _lib.lib()
    assert lib.srt_rebuild_models_abi_version() == 1
    # the additive header leaves the others alone
    assert lib.srt_rebuild_leaf_abi_version() == 1 and lib.srt_rebuild_abi_version() == 1
    assert lib.srt_refit_abi_version() == 1 and lib.srt_query_abi_version() == 1 and lib.srt_abi_version() == 2
    for old in ("srt_rebuild.h", "srt_rebuild_leaf.h"):  # the old headers' out-of-scope lines point here
        assert "srt_rebuild_models.h" in (ROOT / "include" / old).read_text()


def test_scene_shapes(cases):
    """The scenes are what the module says: record counts, a record owning the later block, a leaf root at max_leaf 4."""
    counts = {name: np.bincount(MR.owners(cases[name][0])).tolist() for name in MR.SCENES + MR.EXTRA}
    assert counts == {"two": [1188, 8], "three": [64, 1, 3], "swapped": [1188, 8], "single": [1188], "ones": [1, 1, 1],
                      "nested": [1188, 8]}
    scene, verts, _ = cases["nested"]  # the centre of the grid's box lies inside the cube's box
    p, own = MR.BR.positions(scene, verts), MR.owners(scene)
    centre = (p[own == 1].min((0, 1)) + p[own == 1].max((0, 1))) / 2
    assert (centre > p[own == 0].min((0, 1))).all() and (centre < p[own == 0].max((0, 1))).all()
    own = MR.owners(cases["swapped"][0])
    assert (own[:8] == 1).all() and (own[8:] == 0).all()
    assert int(cases["swapped"][0].bvhs[0]["first_index"]) == 0


@pytest.mark.parametrize("max_leaf", MR.LEAVES)
@pytest.mark.parametrize("name", ALL)
def test_mirror_is_the_single_model_mirror_per_record(cases, name, max_leaf):
    """Nodes, triangles and order equal srt_bvh_build_lbvh_leaf's on every record's triangles alone, concatenated in record
    order (internal references moved by the block's start, leaf references by the segment's)."""
    scene, verts, built = cases[name]
    built, order = built[max_leaf]
    own = MR.owners(scene)
    assert (own >= 0).all()
    node_at = pos = 0
    for r in range(len(scene.bvhs)):
        sub, mine = MR.record_scene(dataclasses.replace(scene, bvhs=scene.bvhs[:1].copy()), own, r)
        alone, o = S.build_lbvh(sub, verts, max_leaf=max_leaf)
        want = alone.nodes.copy()
        leaf = want["count"] > 0
        want["first"] += np.where(leaf, pos, node_at).astype(np.uint32)
        got = built.nodes[node_at:node_at + len(want)]
        assert int(built.bvhs[r]["first_index"]) == node_at and int(built.bvhs[r]["count"]) == len(want)
        assert got.tobytes() == want.tobytes()
        assert (order[pos:pos + len(mine)] == mine[o]).all()
        assert built.tris[pos:pos + len(mine)].tobytes() == alone.tris.tobytes()
        assert (bits(built.bvhs[r]["frame"]) == bits(scene.bvhs[r]["frame"])).all()
        node_at += len(want)
        pos += len(mine)
    assert node_at == len(built.nodes) and pos == len(scene.tris)
    assert (built.tris.tobytes() == scene.tris[order].tobytes()) and sorted(order.tolist()) == list(range(len(order)))
    if name == "three" and max_leaf == 4:
        assert len(MR.blocks(built)[2]) == 1 and int(built.nodes[-1]["count"]) == 3  # the three-triangle model: a leaf root


@pytest.mark.parametrize("max_leaf", MR.LEAVES)
def test_one_record_is_srt_bvh_build_lbvh_leaf_byte_for_byte(cases, max_leaf):
    scene, verts, built = cases["single"]
    built, order = built[max_leaf]
    want, want_order = S.build_lbvh(scene, verts, max_leaf=max_leaf)
    assert built.nodes.tobytes() == want.nodes.tobytes() and built.tris.tobytes() == want.tris.tobytes()
    assert (order == want_order).all() and built.bvhs.tobytes() == want.bvhs.tobytes()


@pytest.mark.parametrize("max_leaf", MR.LEAVES)
@pytest.mark.parametrize("name", ALL)
def test_mirror_agrees_with_the_numpy_rule(cases, name, max_leaf):
    scene, verts, built = cases[name]
    built, order = built[max_leaf]
    own = MR.owners(scene)
    want_order, want_trees = MR.trees(MR.keys(scene, verts, own), own, len(scene.bvhs), max_leaf)
    assert (order == want_order).all()
    first, count = MR.segments(own, len(scene.bvhs))
    for r, nodes in enumerate(MR.blocks(built)):
        assert LR.host_tree(nodes) == want_trees[r], r
    if name == "three":  # 64 equal keys: the tie-break by local position gives the balanced tree over 64 positions
        assert LR.shape(MR.blocks(built)[0])[2] == (6 if max_leaf == 1 else 4)
    # the boxes: srt_bvh_refit's on the mirror's topology
    assert S.refit_scene(built, verts).nodes.tobytes() == built.nodes.tobytes()


@pytest.mark.parametrize("name", MR.SCENES)
def test_oracle_on_the_mirror_equals_the_oracle_on_the_refit_scene(cases, name):
    """Rays started outside every model: the same t bits and the same creation-order triangle on the mirror's arrays as on
    the host-refit scene, with no ray left out (none of these rays meets two triangles at one distance) -- but for the 64
    coincident triangles of scene "three", where any of the 64 is a closest hit: there the record must agree."""
    scene, verts, built = cases[name]
    refit = S.refit_scene(scene, verts)
    rays = MR.scene_rays(scene, verts)
    n = len(scene.bvhs)
    tri_r, t_r, n_r, st = O.Oracle(refit).trace_closest(n, rays)
    assert st["stack_overflow"] == 0
    hit = tri_r != MISS
    assert hit.sum() >= 500 and (~hit).sum() >= 100
    own = MR.owners(scene)
    assert len(set(own[tri_r[hit]].tolist())) == n, "every record is hit"
    for max_leaf in MR.LEAVES:
        b, order = built[max_leaf]
        tri_b, t_b, n_b, st = O.Oracle(b).trace_closest(n, rays)
        assert st["stack_overflow"] == 0
        assert bits_equal(t_b, t_r).all() and bits_equal(n_b, n_r).all()
        got = np.where(tri_b != MISS, order[np.where(tri_b != MISS, tri_b, 0)], MISS)
        assert ((got != MISS) == hit).all()
        same = got == tri_r
        if name == "three":
            same |= hit & (own[np.where(hit, got, 0)] == 0) & (own[np.where(hit, tri_r, 0)] == 0)
            assert (hit & (own[np.where(hit, tri_r, 0)] > 0)).sum() >= 100  # the two small models are compared by triangle
        assert same.all(), f"{(~same).sum()} rays name another triangle"


# -- many records, interleaved records ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MR.MANY + ("many_big",))
def test_many_scene_shapes(cases, name):
    """What rebuild_models_ref.many promises, at the vertices the scenes are rebuilt at: the record count, the cycle of
    triangle counts, the material naming the record, the coincident pairs, the record without extent in z (its key is 0
    on that axis), the 64 equal keys, boxes that stay apart, and the record-bit count the name stands for."""
    scene, verts, built = cases[name]
    R = len(scene.bvhs)
    own = MR.owners(scene)
    assert R == (300 if name == "many_big" else int(name[4:])) and (own >= 0).all() and (np.diff(own) >= 0).all()
    assert len(scene.mats) == R and (scene.tris["mat"] == own).all()
    assert len(np.unique(scene.mats["diffuse"], axis=0)) == R
    special = {MR.AXIS_RECORD: 1, MR.COPIES_RECORD: 64}
    pairs = MR.many_pairs(R)
    count = np.bincount(own)
    p = MR.BR.positions(scene, verts)
    k64 = MR.keys(scene, verts, own)
    for r in range(R):
        source = pairs.get(r, r)
        want = 882 if (name == "many_big" and r == MR.BIG_RECORD) else special.get(source, MR.CYCLE[source % 5])
        assert count[r] == want, r
    assert set(MR.CYCLE) <= set(count[:min(R, 10)].tolist()) or R < 10
    assert len(pairs) == (4 if R >= 80 else R // 20) and all(later > earlier for later, earlier in pairs.items())
    for later, earlier in pairs.items():  # the same corner positions, triangle for triangle, up to the order in the array
        a, b = p[own == later].reshape(-1, 9), p[own == earlier].reshape(-1, 9)
        assert sorted(map(bytes, a)) == sorted(map(bytes, b))
    flat = p[own == MR.AXIS_RECORD]
    assert len(np.unique(flat[..., 2])) == 1 and len(np.unique(flat[..., 0])) > 1 and len(np.unique(flat[..., 1])) > 1
    assert int(k64[own == MR.AXIS_RECORD][0]) & 0x09249249 == 0  # z's bits of the Morton code: ext > 0 is false there
    assert len(np.unique(k64[own == MR.COPIES_RECORD])) == 1
    lo = np.stack([p[own == r].min((0, 1)) for r in range(R)])
    hi = np.stack([p[own == r].max((0, 1)) for r in range(R)])
    apart = (lo[:, None] > hi[None]).any(2) | (hi[:, None] < lo[None]).any(2)
    for later, earlier in pairs.items():
        assert not apart[later, earlier]
        apart[later, earlier] = apart[earlier, later] = True
    assert (apart | np.eye(R, dtype=bool)).all()  # no record inside another, but the coincident ones
    # the sort's end bit: 32 + the least b >= 1 with 2^b >= R
    bits = max(1, int(R - 1).bit_length())
    assert bits == {4: 2, 5: 3, 64: 6, 65: 7, 256: 8, 257: 9, 300: 9}[R]
    assert int(k64.max() >> np.uint64(32)) == R - 1 and (int(k64.max()) >> (32 + bits)) == 0
    if bits > 1:
        assert int(k64.max()) >> (32 + bits - 1) == 1  # one bit less would merge records
    # max_leaf 1 and 4 see leaf roots, records without a pair and real trees
    for L in MR.LEAVES:
        sizes = [len(nodes) for nodes in MR.blocks(built[L][0])]
        assert 1 in sizes and max(sizes) >= 5 and (L > 1 or R < 8 or 3 in sizes)  # (records 6 and 7: two and three triangles)


@pytest.mark.parametrize("name", ("two", "many300", "many_big"))
def test_the_shuffle_interleaves_the_records_and_keeps_the_scene(cases, rubik, name):
    """rebuild_models_ref.shuffled: every triangle is still owned exactly once and by the record that owned it, the owners
    are no longer monotone along the array, and the tree over the moved triangles is the same tree (srt_bvh_refit gives
    the creation boxes back)."""
    scene = cases[name][0]
    got = cases[name + "_shuffled"][0] if name != "two" else MR.shuffled(scene)
    own, own_s = MR.owners(scene), MR.owners(got)  # (owners raises on a triangle met twice)
    assert (own >= 0).all() and (own_s >= 0).all() and (np.diff(own) >= 0).all()
    assert (np.diff(own_s) < 0).sum() >= len(scene.bvhs) // 2 and (np.diff(own_s) != 0).mean() > (0.25 if name != "two" else 0.001)  # (runs of one or two triangles)
    assert sorted(got.tri_input.tolist()) == sorted(scene.tri_input.tolist()) and len(got.tris) == len(scene.tris)
    back = np.argsort(got.tri_input, kind="stable")
    there = np.argsort(scene.tri_input, kind="stable")
    assert got.tris[back].tobytes() == scene.tris[there].tobytes()  # the same triangles under the same loader index
    assert (own_s[back] == own[there]).all()
    assert (got.nodes["count"] == scene.nodes["count"]).all()
    inner = scene.nodes["count"] == 0
    assert (got.nodes["first"][inner] == scene.nodes["first"][inner]).all()
    refit = S.refit_scene(got, got.verts)
    for f in ("min", "max"):
        assert (refit.nodes[f] == scene.nodes[f]).all()
    assert MR.shuffled(scene).tris.tobytes() == got.tris.tobytes()  # a fixed seed


def owner_blocks(scene):
    own = MR.owners(scene)
    return [own[i:i + 256] for i in range(0, len(own), 256)]


def test_blocks_of_one_owner_and_of_many(cases):
    """seg_box_kernel's two paths, from owners() cut into its blocks of 256 triangles.  "many_big" in creation order: blocks
    wholly inside record 150 (the one-owner fold, six atomics a block) and the two that straddle its ends.  Shuffled:
    blocks of a hundred owners and more (six atomics a lane), and in "many_big_shuffled" blocks that record 150's runs
    enter and leave in the middle, none of them one-owner."""
    big = MR.BIG_RECORD
    blocks = owner_blocks(cases["many_big"][0])
    whole = [b for b in blocks if (b == big).all()]
    straddle = [b for b in blocks if (b == big).any() and (b != big).any()]
    assert len(whole) >= 2 and len(straddle) == 2
    assert straddle[0][0] < big and straddle[0][-1] == big and straddle[1][0] == big and straddle[1][-1] > big
    assert all(len(b) == 256 for b in whole)
    mixed = [len(set(b.tolist())) for b in owner_blocks(cases["many300_shuffled"][0])]
    assert len(mixed) >= 4 and min(mixed[:-1]) >= 100
    blocks = owner_blocks(cases["many_big_shuffled"][0])
    assert len(blocks) >= 8 and all(len(set(b.tolist())) > 1 for b in blocks)
    inside = 0
    for b in blocks:
        m = b == big
        enter, leave = np.flatnonzero(~m[:-1] & m[1:]), np.flatnonzero(m[:-1] & ~m[1:])
        inside += len(enter) > 0 and len(leave) > 0 and enter[0] < leave[-1] and len(set(b.tolist())) >= 50
    assert inside >= 4


@pytest.mark.parametrize("name", MR.MANY_HEAVY)
def test_rays_find_every_record_of_the_many(cases, name):
    """The oracle alone, on the mirror-built scenes: every record is srt_hit.bvh of at least one ray -- but the later
    record of each coincident pair, which no ray can find first; the exempt set is stated and at most 5% of R -- the
    earlier record of every pair is found, and the two trees agree on t and on the record of every ray."""
    scene, verts, built = cases[name]
    R = len(scene.bvhs)
    exempt = MR.many_exempt(R)
    assert exempt == ([40, 45, 50, 55] if R >= 80 else []) and len(exempt) <= 0.05 * R
    rays = MR.rays_of(name, scene, verts)
    assert len(rays) == 2000 + MR.MANY_RAYS * R
    found = {}
    for L in MR.LEAVES:
        b, order = built[L]
        tri, t, _, st = O.Oracle(b).trace_closest(R, rays)
        assert st["stack_overflow"] == 0
        hit = tri != MISS
        found[L] = (np.where(hit, MR.bvh_of_position(b)[np.where(hit, tri, 0)], MISS), t)
        seen = set(found[L][0][hit].tolist())
        assert sorted(set(range(R)) - seen) == exempt
        assert all(earlier in seen for earlier in MR.many_pairs(R).values())
    assert (found[1][0] == found[4][0]).all() and bits_equal(found[1][1], found[4][1]).all()


def _mirror_args(scene, verts, max_leaf=1):
    n = len(scene.tris)
    out = dict(bvhs=np.zeros(len(scene.bvhs), S.BVH_DTYPE), nodes=np.zeros(2 * n - 1, S.NODE_DTYPE), n_nodes=C.c_uint32(0),
               tris=np.zeros(n, S.TRI_DTYPE), order=np.full(n, 77, np.uint32))
    args = [S._ptr(scene.bvhs), len(scene.bvhs), S._ptr(scene.nodes), len(scene.nodes), S._ptr(scene.tris), n, S._ptr(verts),
            len(verts), max_leaf, S._ptr(out["bvhs"]), S._ptr(out["nodes"]), C.byref(out["n_nodes"]), S._ptr(out["tris"]),
            S._ptr(out["order"])]
    return args, out


def test_refusals_with_their_messages(cases):
    lib = _lib.lib()
    scene, verts, _ = cases["two"]
    args, out = _mirror_args(scene, verts)
    assert lib.srt_bvh_build_lbvh_models(*args) == _lib.SRT_OK and sorted(out["order"].tolist()) == list(range(len(scene.tris)))

    def refused(s, text, v=verts, max_leaf=1, code=_lib.SRT_ERR_INVALID):
        a, o = _mirror_args(s, v, max_leaf)
        assert lib.srt_bvh_build_lbvh_models(*a) == code
        assert text in _lib.last_error(), _lib.last_error()
        assert (o["order"] == 77).all() and o["n_nodes"].value == 0
        with pytest.raises(S.SrtError):
            S.build_lbvh_models(s, v, max_leaf=max_leaf)

    # a shared triangle: record 1 also starts at record 0's root; and a leaf of record 1 naming a triangle of record 0
    bvhs = scene.bvhs.copy()
    bvhs[1]["first_index"] = 0
    refused(dataclasses.replace(scene, bvhs=bvhs), "every triangle must belong to exactly one BVH record")
    nodes = scene.nodes.copy()
    leaf1 = [j for j in range(int(scene.bvhs[1]["first_index"]), len(nodes)) if nodes[j]["count"] > 0][0]
    nodes[leaf1]["first"], nodes[leaf1]["count"] = 5, 1
    refused(dataclasses.replace(scene, nodes=nodes), "every triangle must belong to exactly one BVH record")
    # an orphan: a triangle no record reaches
    more = np.concatenate([scene.tris, scene.tris[:1]])
    refused(dataclasses.replace(scene, tris=more), "every triangle must belong to exactly one BVH record")
    # record 0 must start at node 0
    refused(dataclasses.replace(scene, bvhs=scene.bvhs[::-1].copy()), "first_index is not 0")
    # the single-model mirror's refusals
    refused(scene, "[1, 255]", max_leaf=0)
    refused(scene, "[1, 255]", max_leaf=256)
    bad = verts.copy()
    bad["pos"][3, 1] = np.inf
    refused(scene, "not finite", v=bad)
    a, o = _mirror_args(scene, verts)
    a[5] = 0
    assert lib.srt_bvh_build_lbvh_models(*a) == _lib.SRT_ERR_INVALID and "at least one triangle" in _lib.last_error()
    for k in (0, 2, 4, 9, 10, 11, 12, 13):
        a, o = _mirror_args(scene, verts)
        a[k] = None
        assert lib.srt_bvh_build_lbvh_models(*a) == _lib.SRT_ERR_INVALID
    # the object call without an object, and the old entry points keep their refusals
    assert lib.srt_query_enable_rebuild_models(None) == _lib.SRT_ERR_INVALID and "null object" in _lib.last_error()
    assert lib.srt_query_enable_rebuild(None) == _lib.SRT_ERR_INVALID and "null object" in _lib.last_error()
    with pytest.raises(ValueError, match="one model"):
        S.build_lbvh(scene, verts)


def test_python_argument_checks_without_a_device(cases):
    from srt_amd.query import Query

    scene = cases["two"][0]
    with pytest.raises(ValueError, match="needs refit=True"):
        Query(scene, rebuild_models=True)
    with pytest.raises(ValueError, match="exclude each other"):
        Query(scene, refit=True, rebuild=True, rebuild_models=True)
    with pytest.raises(ValueError, match="needs rebuild=True"):
        Query(scene, refit=True, rebuild_leaf=4)
    built, order = S.build_lbvh_models(scene, max_leaf=4)  # the scene's own vertices
    assert (bits(built.verts) == bits(scene.verts)).all() and (scene.tri_input[order] == built.tri_input).all()


def test_rebuild_models_host_under_sanitizers():
    """tests/cpp/test_rebuild_models_host.cpp with csrc/rebuild_host.cpp and csrc/refit_host.cpp alone, AddressSanitizer +
    UBSan, as a stand-alone program with its own main (host code only: no HIP, no device, nothing preloaded): the
    package's `make SAN=1 test_rebuild_models_host` builds and runs it."""
    r = subprocess.run(["make", "-s", "-C", str(PKG), "SAN=1", "test_rebuild_models_host"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "rebuild models host checks OK" in r.stdout
    exe = PKG / "build_san" / "test_rebuild_models_host"
    out = subprocess.run(["nm", str(exe)], capture_output=True, text=True, check=True).stdout
    assert "__asan_init" in out and "__ubsan_handle" in out  # the program is instrumented
    assert "hipMalloc" not in out and "BuildLayout" not in out  # host pieces only: no HIP, no query_host.cpp


def test_cpp_mirror_compiles_and_builds_on_the_host():
    """include/srt/query.hpp: Query::EnableRebuildModels and AssetUtils::BuildLBVHModels against the C ABI."""
    out = ROOT / "tests" / "cpp" / "_build"
    out.mkdir(exist_ok=True)
    exe = out / "test_rebuild_models_mirror"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", str(ROOT / "include"),
                    str(ROOT / "tests" / "cpp" / "test_rebuild_models_mirror.cpp"), "-o", str(exe), "-L", str(PKG), "-lsrt_amd",
                    f"-Wl,-rpath,{PKG}"], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "rebuild models mirror OK" in r.stdout, r.stdout + r.stderr
