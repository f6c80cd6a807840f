/*
 * srt_rebuild_leaf.h -- leaves of several triangles for the device rebuild of srt_rebuild.h: every subtree of
 * Karras' hierarchy that covers at most `max_leaf` triangles becomes one leaf, on the device and in the host
 * mirror alike.  The default, max_leaf == 1, is srt_rebuild.h's tree in every dword and every launch.
 *
 * The rule, an extension of rules 4 and 5 of srt_rebuild.h (rules 1-3 -- scene box, key, stable order -- and
 * Karras' hierarchy over the sorted keys are unchanged).  Internal node i of that hierarchy covers the positions
 * [first_i, last_i] and splits after gamma_i; c_i = last_i - first_i + 1.
 *   4a. collapse    for 1 <= max_leaf <= 255: internal node i SURVIVES iff c_i > max_leaf.  A child of a surviving
 *                   node is a leaf (first, count) iff its range holds at most max_leaf positions -- a Karras leaf
 *                   (count 1) or an internal node that does not survive (count = its range) -- and an internal
 *                   reference otherwise.  A parent knows both child ranges from its own split, [first, gamma] and
 *                   [gamma + 1, last]: no node needs another node's result to decide.
 *   4b. numbering   surviving nodes are numbered by increasing Karras index: rank(i) = the number of surviving
 *                   j < i.  Node 0 survives whenever n > max_leaf, so the root is pair 0.  Sibling pair rank(i)
 *                   holds i's children, slot 0 the lower positions.  m, the number of pairs, is the number of
 *                   survivors.  n <= max_leaf gives a leaf root (0, n) and m = 0: the rebuild then reduces to a
 *                   sort and a refit, as n == 1 reduces to a refit.
 *   4c. triangles   inside a leaf keep their sorted positions, which are contiguous: the triangle permutation and
 *                   srt_query_tri_order do not depend on max_leaf.
 *   5.  boxes       and triangle records: srt_refit.h's fold on this topology, unchanged.
 * Depth and heights only shrink against max_leaf == 1; 255 keeps PlanStack's 2-dword packing (leaf counts below
 * 256); max_leaf == 1 is srt_rebuild.h's tree exactly.
 *
 * Out of scope: SAH or any split other than Karras'.  Scenes of more than one BVH record: srt_rebuild_models.h, where
 * this header's max_leaf applies to every record.
 *
 * Additive to srt_rebuild.h and the headers under it (their ABI versions are unchanged); versioned on its own.
 */
#ifndef SRT_REBUILD_LEAF_H
#define SRT_REBUILD_LEAF_H

#include "srt_rebuild.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SRT_REBUILD_LEAF_ABI_VERSION 1

int srt_rebuild_leaf_abi_version(void);                            /* 1 */

/* Sets max_leaf for the object's later rebuilds; it takes effect at the next srt_query_rebuild.  Enqueues nothing.
 * The first value above 1 allocates what the collapse adds on the device (the nodes' ranges, survival flags and
 * ranks, and the scan's temporary storage; "rebuild.leaf_bytes" -- "rebuild.bytes" keeps its value); nothing else
 * allocates.  With max_leaf > 1 a rebuild enqueues a range kernel, hipcub's scan (counted as one launch) and an emit
 * kernel in place of srt_rebuild.h's hierarchy kernel -- "rebuild.launches" is 10 + the refit's where it was 8 + --
 * keeps its one synchronisation, which now also reads m and the largest leaf, and uses the first m of the pair
 * array's n - 1 pairs.  Values may change between rebuilds in either direction: each rebuild's tree is what a fresh
 * object with that value builds.
 * SRT_ERR_INVALID with a message and the state unchanged: a NULL object, an object srt_query_enable_rebuild was
 * not called on, max_leaf == 0 or > 255. */
int srt_query_set_rebuild_leaf(srt_query* q, uint32_t max_leaf);

/* The host mirror: srt_bvh_build_lbvh with rule 4a-4c.  nodes_out has room for 2 * n_tris - 1 nodes; the call
 * writes 2m + 1 of them -- root node 0, the children of pair r at nodes 2r + 1 and 2r + 2 -- and stores that count
 * to *n_nodes_out (a single BVH record with first_index 0 and that count references them).  tris_out and order_out
 * as srt_bvh_build_lbvh writes them.  With max_leaf == 1 every output byte equals srt_bvh_build_lbvh's.
 * Errors as srt_bvh_build_lbvh's (a NULL n_nodes_out included), and SRT_ERR_INVALID for max_leaf == 0 or > 255. */
int srt_bvh_build_lbvh_leaf(const srt_triangle* tris, uint32_t n_tris, const srt_vertex* verts, uint32_t n_verts,
                            uint32_t max_leaf, srt_bvh_node* nodes_out, uint32_t* n_nodes_out, srt_triangle* tris_out,
                            uint32_t* order_out);

/* srt_query_get_int also answers: "rebuild.leaf" (the setting; 1 by default, 0 on an object without rebuild),
 * "rebuild.max_leaf" (the largest leaf of the last rebuild's tree), "rebuild.pairs" (m of the last rebuild) and
 * "rebuild.leaf_bytes" (device bytes srt_query_set_rebuild_leaf allocated).  The existing names keep reporting the
 * tree the object holds: after a collapsed rebuild "layout.pairs" is 64 * max(m, 1), and "refit.*" and "stack.*"
 * describe that tree. */

#ifdef __cplusplus
}
#endif
#endif
