/*
 * srt_rebuild_models.h -- the device rebuild of srt_rebuild.h and srt_rebuild_leaf.h for scenes of several BVH records
 * (the models AssetUtils::UploadModelDataToGPU puts side by side): every record gets the tree the single-model rule
 * builds on that record's triangles alone, in one rebuild over one triangle array, on the device and in the host mirror
 * alike.  A scene of one record enabled here builds, dword for dword and launch for launch, what srt_rebuild.h builds.
 *
 * The rule, stated once; the host function and the device kernels follow it from one text (csrc/rebuild_rule.hpp).
 * R records, n triangles, n_r of them owned by record r.
 *   ownership   triangle t belongs to record r iff t is reachable from r's root in the tree the object was created
 *               with.  Every triangle must belong to exactly one BVH record: a triangle no record reaches, or one two
 *               records reach (instanced records that share nodes), is refused.  bvhs[0].first_index must be 0: the
 *               ghost root (node 0's tree) is record 0's root.  The owner of a triangle is fixed when the rebuild is
 *               enabled; a record's triangles need not be contiguous or in record order in the triangle array.
 *   box, key    rules 1-2 of srt_rebuild.h per record: lo / hi over the owner's triangles only, the same Cell and
 *               Morton.
 *   order       positions sorted by (record, key); equal pairs keep their creation order.  Record r occupies the
 *               positions [s_r, e_r], s_0 = 0, s_(r+1) = e_r + 1 = s_r + n_r: the segments are in record order and
 *               never move.  (The device sorts the 64-bit key (record << 32) | morton with one radix sort.)
 *   hierarchy   rule 4 of srt_rebuild.h inside each segment: Prefix(i, j) is -1 when j lies outside i's own segment,
 *               and the tie-break of equal keys uses segment-local positions, 32 + clz((i - s_r) ^ (j - s_r)).
 *               Karras' node with local index k of record r is pair s_r + k, so r's root is pair s_r; there are
 *               n_r - 1 pairs per record and index e_r is unused.  Root record r references pair s_r.  A record with
 *               n_r == 1, or with n_r <= max_leaf, is a leaf root (s_r, n_r).  Every record owns a triangle: a root is
 *               a leaf of one triangle or more or reaches one, so the case of a record without any cannot arise in
 *               a scene the object or the mirror accepts; both calls refuse it should the walk ever leave one.
 *   collapse    rules 4a-4c of srt_rebuild_leaf.h per record on local ranges (a leaf's first position is global).
 *               Survivors are ranked by increasing global index over all records; m is their total.  max_leaf is
 *               srt_query_set_rebuild_leaf's, which works after either enable.
 *   boxes       and the 48-B triangle records: srt_refit.h's fold through the refit kernels over the new schedule,
 *               every root record and the ghost root included.
 *   depth       the stack plan's depth is the largest over the records.
 * With max_leaf == 1 the pair array keeps its n - 1 slots and the slots e_r in it are zero; with max_leaf > 1 the m
 * pairs are dense, as in srt_rebuild_leaf.h.
 *
 * Out of scope: instanced records (shared nodes or triangles); a changing record, vertex or triangle count; SAH.
 *
 * Additive to srt_rebuild.h and srt_rebuild_leaf.h (their ABI versions, functions and refusals are unchanged:
 * srt_query_enable_rebuild still refuses a scene of several records); versioned on its own.
 */
#ifndef SRT_REBUILD_MODELS_H
#define SRT_REBUILD_MODELS_H

#include "srt_rebuild_leaf.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SRT_REBUILD_MODELS_ABI_VERSION 1

int srt_rebuild_models_abi_version(void);                          /* 1 */

/* srt_query_enable_rebuild for an object of any number of BVH records: the same allocations (with 64-bit sort keys
 * when there are two records or more), plus the owner of every triangle, the record of every position and the segment
 * bounds (all counted in "rebuild.bytes").  The call reads the object's pairs and roots back once to find the owners,
 * and synchronises.  Afterwards srt_query_rebuild, srt_query_set_rebuild_leaf, srt_query_refit, srt_query_closest,
 * srt_query_occluded, srt_query_tri_order and the hit remap work as on a one-record object: srt_hit.triangle stays the
 * creation index and srt_hit.bvh the record; srt_query_update_model_matrix is unaffected (the boxes are in model
 * space); a rebuild still synchronises once.  A second call, or a call after srt_query_enable_rebuild, is SRT_OK and
 * changes nothing.
 * SRT_ERR_INVALID with a message, nothing allocated: a NULL object, an object without SRT_QUERY_REFIT, a record 0
 * whose first_index != 0, a triangle that belongs to no record or to more than one ("every triangle must belong to
 * exactly one BVH record"), a record without a triangle ("every BVH record must own at least one triangle").
 * SRT_ERR_LIMIT: 2^30 triangles or more. */
int srt_query_enable_rebuild_models(srt_query* q);

/* The host mirror.  Record r's nodes form one block of nodes_out, in the layout srt_bvh_build_lbvh_leaf gives that
 * record's triangles alone (the block's root first, the children of its pair k at block nodes 2k + 1 and 2k + 2; child
 * references are indices into nodes_out, leaf references positions in tris_out); the blocks are in record order and
 * bvhs_out[r] is bvhs[r] with first_index the block's start.  tris_out and order_out (position -> input index) hold
 * n_tris entries in (record, key) order; nodes_out has room for 2 * n_tris - 1 nodes and *n_nodes_out is the number
 * written.  `nodes` is only walked to find the owners.  With one record every output equals srt_bvh_build_lbvh_leaf's.
 * Errors: those of srt_bvh_build_lbvh_leaf (a NULL array, n_tris == 0, max_leaf outside [1, 255], a non-finite vertex
 * position, SRT_ERR_LIMIT for n_tris >= 2^30), n_bvhs == 0, a node or triangle reference out of range, and the
 * ownership refusals above, the record without a triangle included. */
int srt_bvh_build_lbvh_models(const srt_bvh_record* bvhs, uint32_t n_bvhs, const srt_bvh_node* nodes, uint32_t n_nodes,
                              const srt_triangle* tris, uint32_t n_tris, const srt_vertex* verts, uint32_t n_verts,
                              uint32_t max_leaf, srt_bvh_record* bvhs_out, srt_bvh_node* nodes_out, uint32_t* n_nodes_out,
                              srt_triangle* tris_out, uint32_t* order_out);

/* srt_query_get_int also answers: "rebuild.models" (1: enabled through srt_query_enable_rebuild_models) and
 * "rebuild.records" (the records the rebuild covers; 1 after srt_query_enable_rebuild) -- both 0 on an object without
 * rebuild.  The existing names keep their meaning and report the last tree: "rebuild.pairs" is m (the pairs of every
 * record together), "rebuild.depth" the largest depth, and with max_leaf == 1 "layout.pairs" stays 64 * (n - 1).
 * "rebuild.height.<h>" (h = 0, 1, ...) is the number of sibling pairs at height h of the last rebuild's tree, as the
 * device counted them for the refit schedule (0 past the last height and before any rebuild; after either enable).
 * "rebuild.launches" of a scene of several records: 7 + the refit's with max_leaf == 1 (one box kernel instead of
 * two), 9 + the refit's above. */

#ifdef __cplusplus
}
#endif
#endif
