/*
 * srt_rebuild.h -- a new BVH for a query object whose mesh has outgrown its refit: a linear BVH (Morton order
 * plus Karras' hierarchy) built on the device from device vertices, and its host mirror.  The object, its refit
 * (srt_refit.h) and the stages that index triangles by srt_hit.triangle carry on as they were.
 *
 * One rule, stated here and followed by the host function and by the device kernels alike.  Every floating
 * point operation is a single rounded fp32 operation: no contraction to FMA, a correctly rounded division.
 *   1. scene box   lo, hi: per component the min and the max over the three vertices of every triangle.  A
 *                  vertex index >= n_verts reads (0,0,0), as elsewhere.  Only the values are used below, so the
 *                  sign of a zero bound cannot matter.
 *   2. key         per component  c = 0.5f * (bmin + bmax)  over the triangle's three vertices,  ext = hi - lo,
 *                  u = ext > 0 ? ((c - lo) / ext) * 1024.0f : 0,  q = min((uint32_t)u, 1023u)  with a
 *                  saturating conversion (u <= 0 or a NaN gives 0, u >= 1023 gives 1023; written as selects, so
 *                  no conversion is out of range on either side).  The 30-bit Morton code interleaves qx, qy,
 *                  qz, x in the highest bit of each triple.
 *   3. order       the triangles sorted by key; equal keys keep their creation order (a stable sort of the
 *                  creation-order sequence, whatever order the object holds them in now).
 *   4. hierarchy   Karras' binary radix tree over the sorted sequence k_0 .. k_(n-1): the common prefix of
 *                  positions i, j is clz(k_i ^ k_j) of the 32-bit keys, and 32 + clz(i ^ j) for equal keys; a
 *                  position outside the sequence has prefix -1.  Every leaf holds exactly one triangle.  The
 *                  children of internal node i form sibling pair i (n - 1 pairs), slot 0 the left child (the
 *                  lower positions) and slot 1 the right; the root is internal node 0.  The prefixes grow
 *                  strictly on the way down and stay below 32 + ceil(log2 n) with at most 30 key bits, so the
 *                  depth is at most 30 + ceil(log2 n): below the 64 entries of the oracle's stack for every
 *                  n < 2^30 the object accepts, and with one-triangle leaves PlanStack's 24-bit packing
 *                  holds while n < 2^24.
 *   5. boxes       and the 48-B triangle records: srt_refit.h's fold, exactly, on the new topology.  The device
 *                  runs the refit kernels over the new schedule for this step.
 * n == 1 keeps a leaf root (the rebuild reduces to a refit); n == 2 is one pair of leaves.
 *
 * Out of scope: SAH (leaves of several triangles by collapsing subtrees: srt_rebuild_leaf.h); a changing n_verts or
 * triangle list.  Scenes of more than one BVH record: srt_rebuild_models.h, whose enable call takes them.
 *
 * Additive to srt_amd.h, srt_query.h and srt_refit.h (their ABI versions are unchanged); versioned on its own.
 */
#ifndef SRT_REBUILD_H
#define SRT_REBUILD_H

#include "srt_refit.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SRT_REBUILD_ABI_VERSION 1

int srt_rebuild_abi_version(void);                                 /* 1 */

/* Attaches the rebuild to an object created with SRT_QUERY_REFIT: allocates its device arrays (the sorted
 * keys and order with the sort's temporary storage, the LBVH's own pairs / index triples / schedule, parents,
 * arrival words and heights; "rebuild.bytes").  Nothing the object held is touched until the first rebuild: its
 * layout, hits and launches stay what they were.  A second call is SRT_OK.
 * SRT_ERR_INVALID with a message: a NULL object, an object without SRT_QUERY_REFIT, a scene of more than one BVH
 * record, a record whose first_index != 0 (one model is the scope: the ghost root then equals the root).
 * SRT_ERR_LIMIT: 2^30 triangles or more. */
int srt_query_enable_rebuild(srt_query* q);

/* Builds the LBVH of the rule above over the object's triangles at verts_dev (as srt_query_refit takes them: a
 * DEVICE array of n_verts 32-B srt_vertex records, 16-B aligned).  On success the object's pairs, roots, tris,
 * index triples, refit schedule and stack plan describe that tree: srt_query_closest, srt_query_occluded and
 * srt_query_refit then work on it, and "stack.*", "refit.heights", "refit.launches", "refit.bytes" and
 * "layout.*" report it.  Runs on the object's stream, in order with the queries there.
 * Unlike srt_query_refit the call is not enqueue-only: it synchronises the stream ONCE, to read the pair counts
 * per height (66 ints at most), and it may reallocate the HBM stack area when the new depth asks for another
 * one (the first rebuild also releases the arrays of the tree it replaces).  verts_dev must stay valid until
 * the call returns.  The device cannot check the vertices: non-finite positions are the caller's contract.
 * SRT_ERR_INVALID, with the state unchanged and nothing enqueued: the failures of srt_query_refit (a NULL
 * object, one created without SRT_QUERY_REFIT, a NULL or misaligned verts_dev, another n_verts than at
 * creation), and an object srt_query_enable_rebuild was not called on.
 *
 * srt_hit.triangle keeps meaning the creation-order triangle index after any number of rebuilds: the rebuild
 * permutes the triangle records, and on a rebuilt object srt_query_closest enqueues one more small launch, one
 * lane per hit, that replaces the record's position by its creation index (misses stay).  An object that was
 * never rebuilt never launches it.  Surface and temporal objects built from the same scene stay valid. */
int srt_query_rebuild(srt_query* q, const srt_vertex* verts_dev, uint32_t n_verts);

/* Test and debug readback of any query object: synchronises, and writes position -> creation index of the
 * triangle records to a HOST array of n == n_tris entries (the identity before any rebuild). */
int srt_query_tri_order(srt_query* q, uint32_t* order_host, uint32_t n);

/* The host mirror: the same tree from HOST arrays.  Writes the std430 node array of 2 * n_tris - 1 nodes
 * (root node 0, the children of internal node i at nodes 2i + 1 and 2i + 2; a single BVH record with
 * first_index 0 references it), the permuted triangle array (n_tris) and the order (position -> input index,
 * n_tris).  These arrays given to srt_query_create, srt_upload_scene or the oracle trace the tree the device
 * builds.  SRT_ERR_INVALID: a NULL array, n_tris == 0, a non-finite vertex position (as srt_bvh_refit);
 * SRT_ERR_LIMIT: n_tris >= 2^30. */
int srt_bvh_build_lbvh(const srt_triangle* tris, uint32_t n_tris, const srt_vertex* verts, uint32_t n_verts,
                       srt_bvh_node* nodes_out, srt_triangle* tris_out, uint32_t* order_out);

/* srt_query_get_int also answers: "rebuild" (1: enabled), "rebuild.count" (rebuilds so far), "rebuild.bytes"
 * (device bytes srt_query_enable_rebuild allocated), "rebuild.launches" (launches of the last rebuild: its own
 * kernels, the sort counted as one, and its refit's) and "rebuild.depth" (depth of the last rebuild's tree) --
 * all 0 on an object without it. */

#ifdef __cplusplus
}
#endif
#endif
