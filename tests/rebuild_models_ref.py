"""A numpy restatement of the several-model rebuild rule (include/srt_rebuild_models.h), for the tests, from the helpers
of tests/rebuild_ref.py and tests/rebuild_leaf_ref.py and not from the C++: the owner of a triangle is the record whose
root reaches it; box and keys per record over its own triangles; positions sorted by (record, key), stable; inside a
record's segment [s, s + n_r) the ranges are split by the prefix rule on the segment's keys and LOCAL positions, and a
side of at most max_leaf positions is a leaf.  Also: the scenes the CPU and GPU tests share, the per-record blocks of
the mirror's node array, and walks of a query object's layout from every root.

Scenes: (a) "two": Rubik beside an 8-triangle grid (refit_ref.grid_triangles(2), moved out of the cube along x);
(b) "three": 64 copies of one triangle (every key equal: local positions decide), a one-triangle model and a
three-triangle model (a leaf root at max_leaf 4); (c) "swapped": (a) with
the two models' triangle blocks exchanged in the triangle array, so record 0 owns the later block; (d) "single": Rubik
alone.  Two more for the structure alone, EXTRA: "ones": three models of one triangle each (no pair at all at max_leaf 1,
the pair array's n - 1 slots all unused); "nested": (a) with the grid where refit_ref.grid_triangles(2) puts it, in the
cube's bottom face -- one record's box overlapping another's, where a box or a key taken over the wrong triangles shows (no ray from
outside reaches the grid first there, which is why (a) moves it).  Every scene is rebuilt at refit_ref.wave(verts, 0.25, 0.3), the amplitude of the one-model tests.
"""
import dataclasses

import numpy as np

import rebuild_leaf_ref as LR
import rebuild_ref as BR
import refit_ref as RR
import srt_amd as S

SCENES = ("two", "three", "swapped", "single")
EXTRA = ("ones", "nested")
GRID_SHIFT = 14.0  # Rubik spans about +-9 around the origin: the grid lies outside it
LEAVES = (1, 4)


def make_scene(name, rubik_model):
    """(scene, verts): the scene a query object is created from and the vertices it is rebuilt at."""
    if name in ("two", "swapped", "nested"):
        shift = 0.0 if name == "nested" else GRID_SHIFT
        grid = RR.grid_triangles(2).reshape(-1, 3, 3) + np.asarray((shift, 0.0, 0.0), np.float32)
        scene = S.Scene.from_models([rubik_model, S.model_from_triangles(grid.reshape(-1, 9))])
        if name == "swapped":
            n0 = len(S.Scene.from_models([rubik_model]).tris)
            n1 = len(scene.tris) - n0
            nodes = scene.nodes.copy()
            leaf = nodes["count"] > 0
            first = nodes["first"].astype(np.int64)
            nodes["first"] = np.where(leaf, np.where(first < n0, first + n1, first - n0), first).astype(np.uint32)
            swap = np.concatenate([np.arange(n0, n0 + n1), np.arange(n0)])
            scene = dataclasses.replace(scene, nodes=nodes, tris=scene.tris[swap].copy(), tri_input=scene.tri_input[swap].copy())
    elif name == "ones":
        grid = RR.grid_triangles(2)
        scene = S.Scene.from_models([S.model_from_triangles(grid[k:k + 1] + 4.0 * k) for k in range(3)])
    elif name == "three":
        grid = RR.grid_triangles(2)
        scene = S.Scene.from_models([S.model_from_triangles(BR.copies_triangles()), S.model_from_triangles(grid[:1] + 3.0),
                                     S.model_from_triangles(grid[:3] - 3.0)])
    else:
        assert name == "single"
        scene = S.Scene.from_models([rubik_model])
    return scene, RR.wave(scene.verts, 0.25, 0.3)


def owners(scene):
    """The record of every triangle (int64; -1: none), by a walk of scene.nodes from every record's root; a triangle met
    twice raises."""
    own = np.full(len(scene.tris), -1, np.int64)
    for r, b in enumerate(scene.bvhs):
        stack = [int(b["first_index"])]
        while stack:
            n = scene.nodes[stack.pop()]
            first, count = int(n["first"]), int(n["count"])
            if count:
                assert (own[first:first + count] == -1).all()
                own[first:first + count] = r
            else:
                stack += [first, first + 1]
    return own


def record_scene(scene, own, r):
    """Record r's triangles in creation order as a scene of their own (the nodes are not used), and their indices."""
    mine = np.flatnonzero(own == r)
    return dataclasses.replace(scene, tris=scene.tris[mine].copy()), mine


def keys(scene, verts, own):
    """(record << 32) | key per triangle (uint64), the key in the owner's box."""
    out = np.zeros(len(scene.tris), np.uint64)
    for r in range(len(scene.bvhs)):
        sub, mine = record_scene(scene, own, r)
        out[mine] = (np.uint64(r) << np.uint64(32)) | BR.keys(sub, verts).astype(np.uint64)
    return out


def segments(own, n_records):
    count = np.bincount(own, minlength=n_records)
    return np.concatenate([[0], np.cumsum(count)[:-1]]), count


def trees(k64, own, n_records, max_leaf):
    """Per record (root, pairs) as rebuild_leaf_ref.collapsed gives them for the segment alone -- local ranks -- with a
    leaf's first position made global."""
    order = np.argsort(k64, kind="stable")
    sorted32 = (k64[order] & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    first, count = segments(own, n_records)
    out = []
    for s, c in zip(first, count):
        root, pairs = LR.collapsed(sorted32[s:s + c], max_leaf)
        shift = lambda ref, s=int(s): ("leaf", ref[1] + s, ref[2]) if ref[0] == "leaf" else ref
        out.append((shift(root), {p: (shift(a), shift(b)) for p, (a, b) in pairs.items()}))
    return order.astype(np.uint32), out


def blocks(built):
    """The mirror's node array cut into the records' blocks, each as a node array of its own (internal references local
    to the block; leaf references stay positions of built.tris)."""
    starts = [int(b["first_index"]) for b in built.bvhs] + [len(built.nodes)]
    assert starts[0] == 0 and all(a < b for a, b in zip(starts, starts[1:]))
    out = []
    for r in range(len(built.bvhs)):
        nodes = built.nodes[starts[r]:starts[r + 1]].copy()
        inner = nodes["count"] == 0
        assert (nodes["first"][inner] > starts[r]).all() and (nodes["first"][inner] + 1 < starts[r + 1]).all()
        nodes["first"][inner] -= starts[r]
        assert int(built.bvhs[r]["count"]) == len(nodes)
        out.append(nodes)
    return out


def walk_nodes(nodes, root):
    """rebuild_ref.walk_nodes from node `root` of a scene's node array."""
    out, stack = [], [(root, "")]
    while stack:
        j, path = stack.pop()
        n = nodes[j]
        box = np.concatenate([n["min"], n["max"]]).view(np.uint32).copy()
        leaf = int(n["count"]) > 0
        out.append((path, leaf, int(n["first"]) if leaf else None, int(n["count"]), box))
        if not leaf:
            stack.append((int(n["first"]) + 1, path + "1"))
            stack.append((int(n["first"]), path + "0"))
    return out


def walk_layout(pairs, roots, r):
    """rebuild_ref.walk_layout from root record r, and the pair indices met (pre-order)."""
    out, met, stack = [], [], [(roots[2 * r], roots[2 * r + 1], "")]
    while stack:
        lo, hi, path = stack.pop()
        ref, cnt = int(lo[3]), int(hi[3])
        out.append((path, cnt > 0, ref if cnt > 0 else None, cnt, np.concatenate([lo[:3], hi[:3]])))
        if cnt == 0:
            met.append(ref)
            p = pairs[4 * ref:4 * ref + 4]
            stack.append((p[2], p[3], path + "1"))
            stack.append((p[0], p[1], path + "0"))
    return out, met


def bvh_of_position(built):
    """The record of every position of built.tris: the segments are in record order."""
    own = owners(built)
    assert (own >= 0).all() and (np.diff(own) >= 0).all()
    return own.astype(np.uint32)


def scene_rays(scene, verts, per_record=700, seed=71):
    """Rays started outside every model -- on a sphere around the whole scene at `verts`, twice its diagonal away: towards
    the whole scene's box, and per record towards points of that record's own box, so that small models are found."""
    from test_gpu_queries import sphere_rays

    p = BR.positions(scene, verts)
    lo, hi = p.reshape(-1, 3).min(0).astype(np.float64), p.reshape(-1, 3).max(0).astype(np.float64)
    sets = [sphere_rays(lo, hi, 2000, seed)]
    own = owners(scene)
    rng = np.random.default_rng(seed + 1)
    for r in range(len(scene.bvhs)):
        q = p[own == r].reshape(-1, 3).astype(np.float64)
        rays = sphere_rays(lo, hi, per_record, seed + 2 + r)
        c, half = (q.min(0) + q.max(0)) / 2, np.maximum((q.max(0) - q.min(0)) / 2, 0.05)
        tgt = c + rng.uniform(-1.2, 1.2, size=(per_record, 3)) * half
        rays["d"] = (tgt - rays["o"].astype(np.float64)).astype(np.float32)
        sets.append(rays)
    return np.concatenate(sets)
