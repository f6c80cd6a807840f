"""Scenes past the size thresholds of the device refit and rebuild, each the smallest that crosses its own, and a numpy
form of the pair array a mirror-built node array stands for.  tests/test_scale_scenes.py holds every scene to what it is
named for with the host mirrors alone; tests/test_gpu_scale.py runs them on the device.

The thresholds and where they come from:
  BOX_LOOP  kBoxBlocks * kBlock of csrc/rebuild.hpp (read from the header): box_partial_kernel's grid-stride loop repeats
            and box_final_kernel folds all kBoxBlocks partial boxes above it;
  ONE_BLOCK, MERGE_LIMIT  rocPRIM's rocprim/device/device_radix_sort.hpp, which hipcub's DeviceRadixSort goes through:
            one block sorts n <= 1,024, a block sort plus merge passes 1,024 < n <= 1,048,576, onesweep above;
  LEVEL     a height of more than 256 pairs gets a launch of its own (csrc/refit.hpp, csrc/scene_refit.hpp);
  in_hbm    a query object's stacks go to HBM when 256 * 3 * 4 * (depth + 1) > 65536 (csrc/query_host.cpp).

"knot70k": render.torus_knot_model(272, 128), 69,632 triangles -- 272 blocks of 256, nodes + triangles over 1 MB.  Its
  triangle array is rotated by whole leaves so that the scene box needs the triangles past the first 65,536.
"clusters": 69,632 triangles, triangle t of scene.tris a copy of base triangle t % 17, base k being
  rebuild_ref.copies_triangles(1) moved 3 k along x: 17 keys of 4,096 triangles each, every key in every block of the
  sort, so only a sort stable across blocks and merge passes gives the mirror's order.  (The loader's own builder would
  group the copies; the creation tree here is a heap of 4,096 leaves of 17 consecutive triangles, boxes by srt_bvh_refit.)
"soup1m": render.synthetic_model(1,052,672): onesweep.
"knot70k_and_rubik": two records, knot70k and Rubik moved outside the knot's box along x; record 0 fills 272 whole
  blocks of seg_box_kernel, Rubik the blocks behind.
"knot70k_and_rubik_shuffled": that scene through rebuild_models_ref.shuffled, the runs of its leaves permuted in the
  triangle array: the two records' triangles interleaved across every block of seg_box_kernel and every tile of the sort.
Every scene but the soup is rebuilt and refit at refit_ref.wave(verts, 0.25, 0.3), as the small tests' scenes are; the
wave moves coincident vertices alike.  The soup is rebuilt where it was created: its midpoint tree gives way to the
linear one all the same.
"""
import dataclasses
import pathlib
import re

import numpy as np

import rebuild_models_ref as MR
import rebuild_ref as BR
import refit_ref as RR
import srt_amd as S
from srt_amd import render as R

ONE_BLOCK = 1024          # rocprim/device/device_radix_sort.hpp: n <= 1,024 is sorted by one block,
MERGE_LIMIT = 1_048_576   # n <= 1,048,576 by a block sort and merge passes, anything larger by onesweep
LEVEL = 256               # pairs of one height above which the refit gives the height a launch of its own
N_KNOT = 2 * 272 * 128    # 69,632
N_BASES = 17
N_SOUP = 1_052_672
LEAVES = (1, 4)           # the max_leaf values tests/test_gpu_scale.py rebuilds at
SCENES = ("knot70k", "clusters", "soup1m", "knot70k_and_rubik", "knot70k_and_rubik_shuffled")


def box_loop_threshold():
    """kBoxBlocks * kBlock, from csrc/rebuild.hpp itself."""
    text = (pathlib.Path(S.__file__).resolve().parent.parent / "csrc" / "rebuild.hpp").read_text()
    value = {name: int(re.search(rf"constexpr uint32_t {name} = (\d+);", text).group(1)) for name in ("kBlock", "kBoxBlocks")}
    return value["kBlock"] * value["kBoxBlocks"]


def cluster_triangles(n=N_KNOT):
    """[n, 9]: triangle t is base t % 17."""
    base = np.concatenate([BR.copies_triangles(1).reshape(1, 3, 3) + np.asarray((3.0 * k, 0.0, 0.0), np.float32)
                           for k in range(N_BASES)])
    return base[np.arange(n) % N_BASES].reshape(-1, 9)


def heap_scene(model, per_leaf):
    """The model's scene with its triangles in the order they were given and, over them, a heap-shaped tree whose leaf j
    holds triangles [per_leaf * j, per_leaf * (j + 1)): node i's children are nodes 2i + 1 and 2i + 2.  The leaf count
    must be a power of two.  The boxes are srt_bvh_refit's."""
    scene = S.Scene.from_models([model])
    n = len(scene.tris)
    leaves = n // per_leaf
    assert leaves * per_leaf == n and leaves >= 2 and leaves & (leaves - 1) == 0
    tris = scene.tris[np.argsort(scene.tri_input, kind="stable")].copy()
    nodes = np.zeros(2 * leaves - 1, scene.nodes.dtype)
    inner = np.arange(leaves - 1)
    nodes["first"][inner] = 2 * inner + 1
    nodes["first"][leaves - 1:] = per_leaf * np.arange(leaves)
    nodes["count"][leaves - 1:] = per_leaf
    bvhs = scene.bvhs.copy()
    bvhs[0]["first_index"], bvhs[0]["count"] = 0, len(nodes)
    scene = dataclasses.replace(scene, bvhs=bvhs, nodes=nodes, tris=tris, tri_input=np.arange(n, dtype=np.uint32))
    return S.refit_scene(scene, scene.verts)


def rolled_so_the_tail_matters(scene, verts, axis=2):
    """`scene` with its triangle array rotated by whole leaves, so that the triangle reaching highest along `axis` at
    `verts` lies in the last leaf of the array: the scene box then depends on the triangles past any shorter prefix, which
    the loader's order does not promise (the knot's box is already that of its first 65,536 triangles)."""
    n = len(scene.tris)
    leaf = np.flatnonzero(scene.nodes["count"] > 0)
    first, count = scene.nodes["first"][leaf].astype(np.int64), scene.nodes["count"][leaf].astype(np.int64)
    top = int(BR.positions(scene, verts)[:, :, axis].max(1).argmax())
    holder = np.flatnonzero((first <= top) & (top < first + count))[0]
    shift = int(n - (first[holder] + count[holder]))
    nodes = scene.nodes.copy()
    nodes["first"][leaf] = (first + shift) % n
    return dataclasses.replace(scene, nodes=nodes, tris=np.roll(scene.tris, shift), tri_input=np.roll(scene.tri_input, shift))


def box_needs_the_tail(scene, verts, head, box=None):
    """Whether the scene box at `verts` differs from the box of the first `head` triangles.  `box`: the scene box (lo, hi)
    where it is known already (a mirror-built tree's root holds it), which spares the gather over every triangle."""
    part = BR.positions(dataclasses.replace(scene, tris=scene.tris[:head]), verts).reshape(-1, 3)
    lo, hi = box if box is not None else BR.scene_box(scene, verts)
    return bool((part.min(0) != lo).any() or (part.max(0) != hi).any())


def knot_and_rubik(rubik_model):
    scene = S.Scene.from_models([R.torus_knot_model(272, 128), rubik_model])
    own = MR.owners(scene)
    mine = np.zeros(len(scene.verts), bool)
    mine[scene.tris["v"][own == 1].reshape(-1)] = True
    assert not mine[scene.tris["v"][own == 0].reshape(-1)].any()  # the records share no vertex
    pos = scene.verts["pos"]
    verts = scene.verts.copy()
    verts["pos"][mine, 0] += np.float32(np.ceil(pos[~mine, 0].max() - pos[mine, 0].min()) + 2.0)
    return S.refit_scene(scene, verts)


def make_scene(name, rubik_model=None):
    """(scene, verts): the scene an object is created from and the vertices it is refit or rebuilt at."""
    if name == "knot70k":
        scene = S.Scene.from_models([R.torus_knot_model(272, 128)])
        scene = rolled_so_the_tail_matters(scene, RR.wave(scene.verts, 0.25, 0.3))
    elif name == "clusters":
        scene = heap_scene(S.model_from_triangles(cluster_triangles()), N_BASES)
    elif name == "soup1m":
        scene = S.Scene.from_models([R.synthetic_model(N_SOUP)])
        return scene, scene.verts  # (no wave: the sort is what this size is for, and the test stays short)
    elif name == "knot70k_and_rubik_shuffled":
        scene = MR.shuffled(knot_and_rubik(rubik_model))
    else:
        assert name == "knot70k_and_rubik"
        scene = knot_and_rubik(rubik_model)
    return scene, RR.wave(scene.verts, 0.25, 0.3)


def leaf255_scene():
    """511 copies of one triangle: at max_leaf 255 the root splits positions [0, 255] from [256, 510], a leaf of 255."""
    scene = S.Scene.from_models([S.model_from_triangles(BR.copies_triangles(511))])
    return scene, RR.wave(scene.verts, 0.25, 0.3)


# -- a node array as the device layout, without a Python loop ------------------------------------------------------------
def pairs_from_nodes(nodes):
    """The uint32 [4 m, 4] pair rows of a mirror-built node array of 2 m + 1 nodes: pair r holds nodes 2r + 1 and
    2r + 2, a node two rows -- (min, reference), (max, count) -- where a leaf's reference is its first position and an
    internal node's the pair of its children, (first - 1) / 2."""
    m = (len(nodes) - 1) // 2
    kids = nodes[1:1 + 2 * m]
    count = kids["count"].astype(np.uint32)
    first = kids["first"].astype(np.uint32)
    out = np.zeros((4 * m, 4), np.uint32)
    out[0::2, :3] = np.ascontiguousarray(kids["min"]).view(np.uint32).reshape(-1, 3)
    out[1::2, :3] = np.ascontiguousarray(kids["max"]).view(np.uint32).reshape(-1, 3)
    out[0::2, 3] = np.where(count > 0, first, (first - np.uint32(1)) // np.uint32(2))
    out[1::2, 3] = count
    return out


def root_from_nodes(nodes, root=0):
    """The two rows of the root record of node `root`, as pairs_from_nodes writes a node."""
    n = nodes[root]
    count, first = int(n["count"]), int(n["first"])
    out = np.zeros((2, 4), np.uint32)
    out[0, :3], out[1, :3] = n["min"].view(np.uint32), n["max"].view(np.uint32)
    out[0, 3], out[1, 3] = (first if count else (first - 1) // 2), count
    return out


def assert_is_a_tree(pairs, m, n_tris):
    """Vectorised: among the rows of the first m pairs every pair but the root's is referenced exactly once and the
    leaves tile [0, n_tris) in reference order."""
    ref, count = pairs[0:4 * m:2, 3].astype(np.int64), pairs[1:4 * m:2, 3].astype(np.int64)
    inner = np.sort(ref[count == 0])
    assert (inner == np.arange(1, m)).all()
    leaf = np.argsort(ref[count > 0], kind="stable")
    first, size = ref[count > 0][leaf], count[count > 0][leaf]
    assert first[0] == 0 and (first[1:] == first[:-1] + size[:-1]).all() and first[-1] + size[-1] == n_tris


def height_counts(nodes):
    """refit_ref.pair_height_counts of a one-record node array whose every node the root reaches, without a Python loop
    over the nodes: heights grow from -1 (a leaf) one level a pass until nothing changes."""
    inner = np.flatnonzero(nodes["count"] == 0)
    first = nodes["first"][inner].astype(np.int64)
    h = np.full(len(nodes), -1, np.int64)
    while len(inner):
        new = 1 + np.maximum(h[first], h[first + 1])
        if (new == h[inner]).all():
            break
        h[inner] = new
    return np.bincount(h[inner]) if len(inner) else np.zeros(0, np.int64)


def schedule_of(counts, limit=LEVEL):
    """(heights, launches of one refit): a launch for the triangles, one for each height under the maximal suffix of
    heights of at most `limit` pairs, and the one-block tail (test_gpu_rebuild.expected_schedule, from the counts)."""
    tail_begin = len(counts)
    while tail_begin > 0 and counts[tail_begin - 1] <= limit:
        tail_begin -= 1
    return len(counts), 2 + tail_begin


def heights_over(scene, limit=LEVEL):
    """The number of heights with more than `limit` sibling pairs."""
    return int((RR.pair_height_counts(scene) > limit).sum())


def in_hbm(depth):
    return 1 if 256 * 3 * 4 * (depth + 1) > 65536 else 0
