"""A numpy restatement of rules 4a-4c of include/srt_rebuild_leaf.h, for the tests, written from the prefix rule of
tests/rebuild_ref.py and not from the C++: walk the ranges from the root; a range [first, last] splits after the last
position g whose prefix with `first` is longer than the range's own; a side that holds at most `max_leaf` positions is one
leaf (first position, count), a larger one is an internal node -- Karras' node g on the left, g + 1 on the right -- and is
walked in turn.  The internal nodes met this way are the survivors; they are numbered by increasing Karras index, and
sibling pair rank(i) holds i's two children, slot 0 the lower positions.
"""
import numpy as np

import rebuild_ref as BR

LEAVES = (1, 2, 3, 4, 8, 255)


def collapsed(k, max_leaf):
    """(root, pairs) over the sorted keys `k`: a reference is ("leaf", first, count) or ("pair", rank); `pairs` maps a
    rank to its (slot 0, slot 1) references.  n <= max_leaf: a leaf root and no pair."""
    n = len(k)
    if n <= max_leaf:
        return ("leaf", 0, n), {}
    found, stack = {}, [(0, 0, n - 1)]
    while stack:
        node, first, last = stack.pop()
        own = BR.prefix(k, first, last)
        g = max(x for x in range(first, last) if BR.prefix(k, first, x) > own)
        sides = []
        for index, a, b in ((g, first, g), (g + 1, g + 1, last)):
            if b - a + 1 <= max_leaf:
                sides.append(("leaf", a, b - a + 1))
            else:
                sides.append(("node", index))
                stack.append((index, a, b))
        found[node] = tuple(sides)
    rank = {node: r for r, node in enumerate(sorted(found))}
    pairs = {rank[node]: tuple(s if s[0] == "leaf" else ("pair", rank[s[1]]) for s in sides) for node, sides in found.items()}
    return ("pair", 0), pairs


def host_tree(nodes):
    """The same (root, pairs) from srt_bvh_build_lbvh_leaf's node array: the children of pair r are nodes 2r + 1, 2r + 2."""
    def ref(j):
        first, count = int(nodes[j]["first"]), int(nodes[j]["count"])
        if count:
            return ("leaf", first, count)
        assert first % 2 == 1 and first + 1 < len(nodes)
        return ("pair", (first - 1) // 2)
    assert len(nodes) % 2 == 1
    return ref(0), {r: (ref(2 * r + 1), ref(2 * r + 2)) for r in range((len(nodes) - 1) // 2)}


def shape(nodes):
    """(m, largest leaf, depth) of a host-built node array; a leaf root has depth 0."""
    depth, stack = 0, [(0, 0)]
    while stack:
        j, d = stack.pop()
        depth = max(depth, d)
        if int(nodes[j]["count"]) == 0:
            stack += [(int(nodes[j]["first"]), d + 1), (int(nodes[j]["first"]) + 1, d + 1)]
    return (len(nodes) - 1) // 2, int(nodes["count"].max()), depth


def leaf_sizes(nodes):
    """Triangles under every node of the array (int64): a walk from the root, summed on the way back."""
    size = nodes["count"].astype(np.int64)
    order, stack = [], [0]
    while stack:
        j = stack.pop()
        if nodes[j]["count"] == 0:
            order.append(j)
            stack += [int(nodes[j]["first"]), int(nodes[j]["first"]) + 1]
    for j in reversed(order):  # (a child is met after its parent)
        c = int(nodes[j]["first"])
        size[j] = size[c] + size[c + 1]
    return size
