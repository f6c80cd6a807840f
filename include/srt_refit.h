/*
 * srt_refit.h -- BVH refit for meshes whose vertices move: the topology stays, the boxes and the query
 * object's precomputed triangle records follow the new vertices.
 *
 * One rule, stated here and used by the host function and by the device kernels alike:
 *   leaf box      fold over the leaf's triangles first .. first+count-1 in order, and within a triangle over
 *                 v0, v1, v2, starting from the first vertex; per component  m = v < m ? v : m  for the min and
 *                 m = v > m ? v : m  for the max.  A vertex index >= n_verts reads (0,0,0).
 *   internal box  child 0's box folded with child 1's by the same two expressions.
 * The fold order fixes the sign of a zero bound, so the results are comparable bit for bit.  The reference's
 * builder makes its boxes the same way (UpdateNodeBounds, bvh.h:80-95: a pure min/max over the primitives'
 * vertices), so a refit at unchanged vertices reproduces the built boxes as values.
 *
 * Out of scope:
 *   - a new topology (srt_rebuild.h builds one on the device for a query object) and a changing n_verts;
 *   - motion of lights.
 *
 * The path tracer's own device scene follows the same rule through srt_scene_refit.h (srt_upload_scene_refit,
 * then srt_scene_refit per frame), which replaces srt_bvh_refit + srt_upload_scene in a frame loop.
 *
 * Additive to srt_amd.h and srt_query.h (SRT_ABI_VERSION and SRT_QUERY_ABI_VERSION are unchanged); versioned
 * on its own.
 */
#ifndef SRT_REFIT_H
#define SRT_REFIT_H

#include "srt_query.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SRT_REFIT_ABI_VERSION 1
#define SRT_QUERY_REFIT 1u   /* srt_query_create_ex flag: the object can be refit */

int srt_refit_abi_version(void);                                   /* 1 */

/* Host refit, in place.  Validates as srt_query_create does (SRT_ERR_INVALID: a BVH root, child or triangle
 * index out of range, a cycle, a leaf count >= 2^31) and rejects a non-finite vertex position; on failure
 * `nodes` is untouched.  Then rewrites min_bounds / max_bounds of every node some traversal reaches (from a
 * BVH record's first_index, or from node 0) by the rule above.  Nodes no traversal reaches, and every
 * first_child_or_prim_index and prim_count, are left alone. */
int srt_bvh_refit(const srt_bvh_record* bvhs, uint32_t n_bvhs, srt_bvh_node* nodes, uint32_t n_nodes,
                  const srt_triangle* tris, uint32_t n_tris, const srt_vertex* verts, uint32_t n_verts);

/* srt_query_create / srt_query_create_obj with flags; flags == 0 is exactly those calls.  With
 * SRT_QUERY_REFIT the object also keeps, on the device, the triangles' vertex indices (16 B a triangle) and
 * a refit schedule (4 B a sibling pair, plus the offsets of the levels one block walks). */
int srt_query_create_ex(int device, void* stream,
                        const srt_bvh_record* bvhs, uint32_t n_bvhs, const srt_bvh_node* nodes, uint32_t n_nodes,
                        const srt_triangle* tris, uint32_t n_tris, const srt_vertex* verts, uint32_t n_verts,
                        uint32_t flags, srt_query** out);
int srt_query_create_obj_ex(int device, void* stream, const srt_scene* s, uint32_t flags, srt_query** out);

/* Refits the object's device scene to verts_dev: a DEVICE array of n_verts 32-B srt_vertex records, 16-B
 * aligned, on the query's device (the kernels read the first 16 B of each).  Afterwards the device arrays
 * equal, in every dword, what srt_query_create uploads for the nodes srt_bvh_refit yields with these
 * vertices.  The call only enqueues on the query's stream, ordered with the queries there: no allocation,
 * no synchronisation, no host copy; verts_dev must stay valid until that work has run.  The device cannot
 * check the vertices: non-finite positions are the caller's contract.
 * SRT_ERR_INVALID, with the state unchanged and nothing enqueued: a NULL object, an object created without
 * SRT_QUERY_REFIT, a NULL or misaligned verts_dev, n_verts different from the count at creation. */
int srt_query_refit(srt_query* q, const srt_vertex* verts_dev, uint32_t n_verts);

/* Test and debug readback of any query object: synchronises the stream and copies the device arrays of
 * csrc/query_host.hpp's layout to HOST buffers of "layout.pairs" / "layout.roots" / "layout.tris" bytes
 * (srt_query_get_int).  NULL skips an array. */
int srt_query_copy_layout(srt_query* q, void* pairs, void* roots, void* tris);

/* srt_query_get_int also answers: "refit" (1: created with SRT_QUERY_REFIT), "refit.heights" (levels of the
 * schedule), "refit.launches" (kernel launches of one srt_query_refit), "refit.bytes" (device bytes of the
 * vertex indices and the schedule; no part of "scratch.bytes"), "refit.count" (refits enqueued so far) --
 * all 0 without the flag -- and "layout.pairs" / "layout.roots" / "layout.tris" on every object. */

#ifdef __cplusplus
}
#endif
#endif
