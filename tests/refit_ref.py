"""A numpy restatement of the refit rule (include/srt_refit.h), for the tests: the node boxes of a scene at new
vertices, the layout a query object holds for them, and the deterministic deformation the tests share.

Leaf box: fold over the leaf's triangles first .. first+count-1 in order, within a triangle over v0, v1, v2, starting
from the first vertex; ``m = v < m ? v : m`` for the min, ``m = v > m ? v : m`` for the max; a vertex index past the
array reads (0, 0, 0).  Internal box: child 0's box folded with child 1's by the same two expressions.
"""
import numpy as np

import srt_amd as S

# Sine amplitude of `wave` on Rubik (about 18 units across): the oracle alone sees every one of 4099 rubik_rays that
# hits both meshes change t, and 10% change triangle or hit/miss (0.1 gives 4.6%, under the 5% the GPU test asks).
WAVE_AMPLITUDE = 0.25


def wave(scene_verts, amplitude=WAVE_AMPLITUDE, phase=0.0):
    """A VERT_DTYPE copy displaced by a sine of each vertex's own position (float32 arithmetic, deterministic)."""
    from srt_amd import render as R

    return R.wave_vertices(scene_verts, amplitude, phase)


def grid_triangles(n=24, seed=3, jitter=0.45):
    """n x n quads (2 n^2 triangles) over [0, n]^2 with a bumpy height, the corners jittered in the plane: xyz9 rows
    for model_from_triangles.  The jitter matters at n = 24: the midpoint splits of a regular grid give exactly 256
    sibling pairs of two leaves, and the refit's one-block tail would take every level; this one has 272."""
    rng = np.random.default_rng(seed)
    z = rng.uniform(-0.4, 0.4, size=(n + 1, n + 1)).astype(np.float32)
    dx = rng.uniform(-jitter, jitter, size=(n + 1, n + 1))
    dy = rng.uniform(-jitter, jitter, size=(n + 1, n + 1))
    tri = []
    for j in range(n):
        for i in range(n):
            c = [(a + dx[b, a], b + dy[b, a], z[b, a]) for a, b in ((i, j), (i + 1, j), (i + 1, j + 1), (i, j + 1))]
            tri.append([c[0], c[1], c[2]])
            tri.append([c[0], c[2], c[3]])
    return np.asarray(tri, np.float32).reshape(-1, 9)


def pair_height_counts(scene):
    """Sibling pairs per height (0: both children leaves, else 1 + the largest height of its internal children),
    from the nodes alone: an internal node owns the pair of its children."""
    n, h = scene.nodes, {}
    stack = [int(b["first_index"]) for b in scene.bvhs] + [0]
    while stack:
        j = stack[-1]
        c = int(n[j]["first"])
        if n[j]["count"] > 0:
            h[j] = -1
        elif c in h and c + 1 in h:
            h[j] = 1 + max(h[c], h[c + 1])
        else:
            stack += [k for k in (c, c + 1) if k not in h]
            continue
        stack.pop()
    return np.bincount(np.array([v for v in h.values() if v >= 0], np.int64))


def _fold_min(m, v):
    return np.where(v < m, v, m)


def _fold_max(m, v):
    return np.where(v > m, v, m)


def leaf_box(tris, verts, first, count):
    pos = np.concatenate([verts["pos"].astype(np.float32), np.zeros((1, 3), np.float32)])  # the last row: out of range
    idx = tris["v"][first:first + count].reshape(-1).astype(np.int64)
    idx = np.where(idx < len(verts), idx, len(verts))
    lo = hi = pos[idx[0]]
    for i in idx:
        lo, hi = _fold_min(lo, pos[i]), _fold_max(hi, pos[i])
    return lo, hi


def refit_nodes(scene, verts):
    """`scene.nodes` refit to `verts`: a copy; nodes no traversal reaches and every index field as they were."""
    nodes = scene.nodes.copy()
    done = np.zeros(len(nodes), bool)
    for root in [int(b["first_index"]) for b in scene.bvhs] + [0]:
        stack = [(root, False)]
        while stack:
            i, children_done = stack.pop()
            if done[i]:
                continue
            first, count = int(nodes[i]["first"]), int(nodes[i]["count"])
            if count > 0:
                nodes[i]["min"], nodes[i]["max"] = leaf_box(scene.tris, verts, first, count)
            elif not children_done:
                stack += [(i, True), (first, False), (first + 1, False)]
                continue
            else:
                nodes[i]["min"] = _fold_min(nodes[first]["min"], nodes[first + 1]["min"])
                nodes[i]["max"] = _fold_max(nodes[first]["max"], nodes[first + 1]["max"])
            done[i] = True
    return nodes


def reached(scene):
    """Mask of the nodes some traversal reaches (from the BVH records' roots and from node 0)."""
    seen = np.zeros(len(scene.nodes), bool)
    stack = [int(b["first_index"]) for b in scene.bvhs] + [0]
    while stack:
        i = stack.pop()
        if seen[i]:
            continue
        seen[i] = True
        if scene.nodes[i]["count"] == 0:
            stack += [int(scene.nodes[i]["first"]), int(scene.nodes[i]["first"]) + 1]
    return seen


def rebuilt_scene(scene, verts):
    """A scene BUILT from the deformed triangles: the same float positions, in the flattened scene's triangle order."""
    xyz9 = verts["pos"][scene.tris["v"]].reshape(-1, 9)
    return S.Scene.from_models([S.model_from_triangles(xyz9)])
