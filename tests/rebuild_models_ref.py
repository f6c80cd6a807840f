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

Many records, MANY and MANY_MIXED: "many<R>" for R of MANY_R, R small models of 1, 2, 3, 5 and 9 triangles on a jittered
lattice, each with a material of its own, among them a triangle without extent in z, 64 coincident triangles and pairs of
records that coincide (many_triangles); "many_big": many300 with record 150 a grid of 882 triangles, so that in creation
order some 256-triangle blocks of seg_box_kernel lie inside one record and two straddle its ends; and "many300_shuffled",
"many_big_shuffled": those two through `shuffled`, the leaves' runs permuted in the triangle array, so that consecutive
triangles belong to different records.
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

# -- many records --------------------------------------------------------------------------------------------------------
# many(R): R small models on a jittered lattice, one material each.  R steps over the record-bit counts of the sort's end
# bit (4 | 5: 2 | 3 bits, 64 | 65: 6 | 7, 256 | 257: 8 | 9, the last past one 8-bit radix digit above bit 32) and over the
# 256 lanes of the refit's roots loop (n_roots = R + 1: 257, 258, 301).
MANY_R = (4, 5, 64, 65, 256, 257, 300)
MANY = tuple(f"many{R}" for R in MANY_R)                     # the rule-level tests
MANY_MIXED = ("many_big", "many300_shuffled", "many_big_shuffled")
MANY_HEAVY = ("many5", "many257", "many300") + MANY_MIXED    # hits, stages, refit
# scene_rays' per_record for these scenes.  A ray aimed into the box of a one-triangle model meets the triangle about one
# time in seven, so 24 a record leave one record in a hundred unfound (the oracle alone shows it); 64 find every record
# three times and more.  21 k rays at 300 records: a third of a second of the oracle per tree.
MANY_RAYS = 64
CYCLE = (1, 2, 3, 5, 9)
SPACING, JITTER = 12.0, 2.0  # the models are pieces of grid_triangles(3), at most 3.9 across: boxes 4.1 apart at least,
#   and sparse enough that rays from outside find the inner ones
AXIS_RECORD, COPIES_RECORD = 1, 2
BIG_RECORD, BIG_GRID = 150, 21  # grid_triangles(21): 882 triangles, at least 3 * 256 + 100 and under the restatement's 1 000
SHUFFLE_SEED = 17


def many_pairs(R):
    """{later record: earlier record} of the records with identical geometry at identical positions: four pairs over the
    cycle's counts 5, 9, 1 and 3 from R = 80 on, and below as many of them as stay under 5% of R (three at 64 and 65, none
    at 4 and 5): no ray finds the later record of a pair first, and the rays must find all but 5% of the records."""
    return dict(list({40: 3, 45: 4, 50: 5, 55: 7}.items())[:min(4, R // 20)])


def many_triangles(R, big=False):
    """Per record its xyz9 rows.  Record k: CYCLE[k % 5] triangles of refit_ref.grid_triangles(3) from row k % 7 on, at
    lattice point k of a cube of ceil(cbrt(R)) points a side, jittered (seed 29); but record 1 one triangle in a plane
    z = const (no extent in z), record 2 rebuild_ref.copies_triangles() -- 64 coincident triangles -- and the later record
    of every pair of many_pairs the earlier one's rows.  `big`: record BIG_RECORD a bumped grid beside the lattice."""
    base = RR.grid_triangles(3)
    side = int(np.ceil(R ** (1.0 / 3.0) - 1e-9))
    rng = np.random.default_rng(29)
    jitter = rng.uniform(-JITTER, JITTER, size=(R, 3))
    out = []
    for k in range(R):
        at = (SPACING * np.asarray((k % side, (k // side) % side, k // (side * side))) + jitter[k]).astype(np.float32)
        if k == AXIS_RECORD:
            tri = np.asarray([[0.25, 0.5, 1.0, 2.5, 0.75, 1.0, 1.0, 3.0, 1.0]], np.float32)
        elif k == COPIES_RECORD:
            tri = BR.copies_triangles()
        else:
            tri = base[k % 7:k % 7 + CYCLE[k % len(CYCLE)]]
        out.append((tri.reshape(-1, 3, 3) + at).reshape(-1, 9))
    if big:
        tri = RR.grid_triangles(BIG_GRID).reshape(-1, 3, 3).copy()
        x, y = tri[:, :, 0], tri[:, :, 1]  # lifted as rebuild_ref.bump lifts vertices
        tri[:, :, 2] = (tri[:, :, 2] + np.float32(0.6) * np.sin(np.float32(0.7) * x + np.float32(0.3)) * np.cos(np.float32(0.5) * y))
        out[BIG_RECORD] = (tri.astype(np.float32) - np.asarray((BIG_GRID + 5.0, 0.0, 0.0), np.float32)).reshape(-1, 9)
    for later, earlier in many_pairs(R).items():
        out[later] = out[earlier].copy()
    return out


def many_kd(k):
    """Record k's diffuse colour: one of 8^3, so the material -- and the albedo a surface stage reads -- names the record."""
    return ((k % 8 + 1) / 8.0, (k // 8 % 8 + 1) / 8.0, (k // 64 + 1) / 8.0)


def many(R, big=False):
    """(scene, verts): the R models in record order, every triangle's material its record; rebuilt at the wave of every
    other scene, with record 1's three vertices put back into one plane z = const (the wave moves z by a sine of x and y)."""
    scene = S.Scene.from_models([S.model_from_triangles(tri, kd=many_kd(k)) for k, tri in enumerate(many_triangles(R, big))])
    verts = RR.wave(scene.verts, 0.25, 0.3)
    flat = scene.tris["v"][owners(scene) == AXIS_RECORD].reshape(-1)
    verts["pos"][flat, 2] = verts["pos"][flat[0], 2]
    return scene, verts


def leaf_runs(scene):
    """The (first, count) runs of the leaves reachable from every record's root, in the order of the walk."""
    runs = []
    for b in scene.bvhs:
        stack = [int(b["first_index"])]
        while stack:
            j = stack.pop()
            first, count = int(scene.nodes[j]["first"]), int(scene.nodes[j]["count"])
            if count:
                runs.append((j, first, count))
            else:
                stack += [first + 1, first]
    return runs


def shuffled(scene, seed=SHUFFLE_SEED):
    """`scene` with the runs of its leaves permuted in the triangle array (what "swapped" does for two blocks, per leaf):
    tris and tri_input move, every leaf's `first` follows.  The same records own the same triangles, but consecutive
    triangles of the array now belong to different records."""
    runs = leaf_runs(scene)
    nodes = scene.nodes.copy()
    src, at = [], 0
    for k in np.random.default_rng(seed).permutation(len(runs)):
        j, first, count = runs[k]
        nodes[j]["first"] = at
        src.append(np.arange(first, first + count))
        at += count
    src = np.concatenate(src)
    assert at == len(scene.tris) and (np.sort(src) == np.arange(at)).all()  # the leaves tile the array
    return dataclasses.replace(scene, nodes=nodes, tris=scene.tris[src].copy(), tri_input=scene.tri_input[src].copy())


def many_scene(name):
    """The scene of a name of MANY or MANY_MIXED."""
    core = name[:-len("_shuffled")] if name.endswith("_shuffled") else name
    scene, verts = many(300, big=True) if core == "many_big" else many(int(core[len("many"):]))
    return (shuffled(scene) if core != name else scene), verts


def many_exempt(R):
    """The records of many(R) no ray from outside finds first: the later record of every coincident pair (the earlier one
    is visited first and keeps the hit).  The construction places no record inside another."""
    return sorted(many_pairs(R))


def rays_of(name, scene, verts):
    """scene_rays, with MANY_RAYS a record on the many-record scenes."""
    return scene_rays(scene, verts, per_record=MANY_RAYS) if name.startswith("many") else scene_rays(scene, verts)


def make_scene(name, rubik_model):
    """(scene, verts): the scene a query object is created from and the vertices it is rebuilt at."""
    if name.startswith("many"):
        return many_scene(name)
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
