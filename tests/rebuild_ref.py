"""A numpy restatement of the rebuild rule (include/srt_rebuild.h), for the tests: the scene box, the Morton keys, the
stable order and -- directly from the prefix rule, a scan per node -- the hierarchy; walks of the host-built node array
and of a query object's device layout; and the scenes the CPU and GPU tests share.

Key: per component c = 0.5f * (bmin + bmax) of the triangle's vertices, ext = hi - lo, u = ext > 0 ? ((c - lo) / ext) *
1024.0f : 0, q = min((uint32_t)u, 1023) saturating; the 30-bit code interleaves qx qy qz, x highest.  Prefix of positions
i, j of the sorted keys: clz(k_i ^ k_j), and 32 + clz(i ^ j) for equal keys.  A range [first, last] splits after the last
position g whose prefix with `first` is longer than the range's own; its left child is internal node g (or leaf g when
that side is one position), its right child internal node g + 1 (or leaf g + 1); the root is internal node 0.
"""
import dataclasses

import numpy as np

import refit_ref as RR
import srt_amd as S

F = np.float32


def positions(scene, verts):
    """[n_tris, 3, 3] float32 corner positions; a vertex index past the array reads (0, 0, 0)."""
    pos = np.concatenate([np.asarray(verts["pos"], F), np.zeros((1, 3), F)])
    idx = scene.tris["v"].astype(np.int64)
    return pos[np.where(idx < len(verts), idx, len(verts))]


def scene_box(scene, verts):
    p = positions(scene, verts).reshape(-1, 3)
    return p.min(0), p.max(0)


def spread3(x):
    x = x.astype(np.uint64)
    x = (x * 0x00010001) & 0xFF0000FF
    x = (x * 0x00000101) & 0x0F00F00F
    x = (x * 0x00000011) & 0xC30C30C3
    x = (x * 0x00000005) & 0x49249249
    return x.astype(np.uint32)


def keys(scene, verts):
    """The key of every triangle, in the scene's order (uint32)."""
    p = positions(scene, verts)
    lo, hi = scene_box(scene, verts)
    bmin, bmax = p.min(1), p.max(1)
    with np.errstate(all="ignore"):
        c = (F(0.5) * (bmin + bmax)).astype(F)
        ext = (hi - lo).astype(F)
        u = (((c - lo).astype(F) / ext).astype(F) * F(1024.0)).astype(F)
        u = np.where(ext > 0, u, F(0))
        q = np.where(~(u > 0), 0, np.where(u >= 1023, 1023, np.clip(np.nan_to_num(u), 0, 1023).astype(np.uint32)))
    q = q.astype(np.uint32)
    return (spread3(q[:, 0]) << 2) | (spread3(q[:, 1]) << 1) | spread3(q[:, 2])


def order(k):
    return np.argsort(k, kind="stable").astype(np.uint32)


def _clz32(x):
    return 32 - int(x).bit_length()


def prefix(k, i, j):
    x = int(k[i]) ^ int(k[j])
    if x:
        return _clz32(x)
    return 32 + _clz32(i ^ j) if i != j else 64


def hierarchy(k):
    """{internal node: ((index, is_leaf), (index, is_leaf))} over the sorted keys `k`, by the prefix rule alone."""
    n, out = len(k), {}
    stack = [(0, 0, n - 1)] if n > 1 else []
    while stack:
        node, first, last = stack.pop()
        own = prefix(k, first, last)
        g = max(x for x in range(first, last) if prefix(k, first, x) > own)
        left = (g, first == g)
        right = (g + 1, last == g + 1)
        out[node] = (left, right)
        if not left[1]:
            stack.append((g, first, g))
        if not right[1]:
            stack.append((g + 1, g + 1, last))
    return out


def host_children(nodes):
    """The same dict from srt_bvh_build_lbvh's node array: the children of internal node i are nodes 2i + 1, 2i + 2."""
    def ref(j):
        first, count = int(nodes[j]["first"]), int(nodes[j]["count"])
        assert count in (0, 1)
        if count:
            return (first, True)
        assert first % 2 == 1
        return ((first - 1) // 2, False)
    return {i: (ref(2 * i + 1), ref(2 * i + 2)) for i in range((len(nodes) - 1) // 2)}


def walk_nodes(nodes):
    """A pre-order list of (path, is_leaf, first triangle or None, count, box dwords[6]) of a std430 node array."""
    out, stack = [], [(0, "")]
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


def walk_layout(pairs, roots):
    """The same list from a query object's device layout (Query.layout(): uint32 [n, 4] rows), from root record 0."""
    out, stack = [], [(roots[0], roots[1], "")]
    while stack:
        lo, hi, path = stack.pop()
        ref, cnt = int(lo[3]), int(hi[3])
        box = np.concatenate([lo[:3], hi[:3]])
        out.append((path, cnt > 0, ref if cnt > 0 else None, cnt, box))
        if cnt == 0:
            p = pairs[4 * ref:4 * ref + 4]
            stack.append((p[2], p[3], path + "1"))
            stack.append((p[0], p[1], path + "0"))
    return out


def assert_same_tree(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g[:4] == w[:4], (g[:4], w[:4])
        assert (g[4] == w[4]).all(), (g[0], g[4], w[4])


def layout_tris(scene):
    """The 48-B triangle records query_host.hpp's layout holds for `scene` (uint32 [3 (n + 1), 4]): v0, e1, e2,
    material, position, 0, and the zero pad record."""
    p = positions(scene, scene.verts)
    n = len(scene.tris)
    rec = np.zeros((n + 1, 12), F)
    rec[:n, 0:3] = p[:, 0]
    rec[:n, 3:6] = p[:, 1] - p[:, 0]
    rec[:n, 6:9] = p[:, 2] - p[:, 0]
    rec = rec.view(np.uint32)
    rec[:n, 9] = scene.tris["mat"]
    rec[:n, 10] = np.arange(n, dtype=np.uint32)
    return rec.reshape(-1, 4)


# -- the scenes ---------------------------------------------------------------------------------------------------------
def flat_grid_triangles(n=24):
    """refit_ref.grid_triangles with every height zero: before a displacement the scene box has no extent in z."""
    tri = RR.grid_triangles(n).reshape(-1, 3, 3).copy()
    tri[:, :, 2] = 0.0
    return tri.reshape(-1, 9)


def copies_triangles(n=64):
    return np.tile(np.asarray([[0.5, 0.25, 1.0, 2.5, 0.75, 1.5, 1.0, 3.0, -0.5]], F), (n, 1))


def bump(verts, amplitude=0.6):
    """A VERT_DTYPE copy lifted in z by a sine of x and y (float32, deterministic): makes a flat mesh a surface."""
    v = verts.copy()
    p = v["pos"]
    v["pos"][:, 2] = (p[:, 2] + F(amplitude) * np.sin(F(0.7) * p[:, 0] + F(0.3)) * np.cos(F(0.5) * p[:, 1])).astype(F)
    return v


SCENES = ("rubik", "grid", "grid_flat", "copies", "one", "two", "three", "oob")


def make_scene(name, rubik_model):
    """(scene, verts): the scene a query object is created from and the vertices it is rebuilt at."""
    if name == "rubik":
        scene = S.Scene.from_models([rubik_model])
        return scene, RR.wave(scene.verts, 0.25, 0.3)
    if name in ("grid", "grid_flat"):
        scene = S.Scene.from_models([S.model_from_triangles(flat_grid_triangles())])
        return scene, (bump(scene.verts) if name == "grid" else scene.verts.copy())
    if name == "copies":
        scene = S.Scene.from_models([S.model_from_triangles(copies_triangles())])
        return scene, RR.wave(scene.verts, 0.25, 0.3)
    if name in ("one", "two", "three"):
        k = {"one": 1, "two": 2, "three": 3}[name]
        scene = S.Scene.from_models([S.model_from_triangles(RR.grid_triangles(2)[:k])])
        return scene, RR.wave(scene.verts, 0.25, 0.3)
    assert name == "oob"
    scene = S.Scene.from_models([S.model_from_triangles(RR.grid_triangles(3))])
    tris = scene.tris.copy()
    tris["v"][5, 1] = len(scene.verts) + 7  # reads (0, 0, 0): the grid lies in [0, 3]^2, so the box grows
    tris["v"][11, 0] = 0xFFFFFFF0
    scene = S.refit_scene(dataclasses.replace(scene, tris=tris), scene.verts)
    verts = scene.verts.copy()
    verts["pos"] += F(2.0)  # away from the origin: the out-of-range corners stay at (0, 0, 0)
    return scene, verts
