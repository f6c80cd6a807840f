/*
 * srt_scene_refit.h -- refit of the path tracer's own device scene when a mesh's vertices move: the topology,
 * the device layout and every size stay, the node boxes and the triangle records follow vertices that already
 * live on the device.  The rule is srt_refit.h's fold, so the result is comparable bit for bit with the host
 * path (srt_bvh_refit, then srt_upload_scene of the refit nodes), which this call replaces in a frame loop.
 *
 * Out of scope:
 *   - srt_group / GroupRenderer: an object per context works;
 *   - rebuilds, topology changes and a changing n_verts;
 *   - motion of lights;
 *   - the pool and wavefront modes beyond keeping the treelet copy of the node array equal to the host path's.
 *
 * Additive to srt_amd.h and srt_refit.h (SRT_ABI_VERSION and SRT_REFIT_ABI_VERSION are unchanged); versioned
 * on its own.
 */
#ifndef SRT_SCENE_REFIT_H
#define SRT_SCENE_REFIT_H

#include <stddef.h>

#include "srt_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SRT_SCENE_REFIT_ABI_VERSION 1

int srt_scene_refit_abi_version(void);                             /* 1 */

/* The object's type shares its name with the call that uses it, so it has no typedef: it is always written
 * `struct srt_scene_refit` (a tag, which C keeps apart from function names and C++ finds behind one). */
struct srt_scene_refit;

/* srt_upload_scene with exactly these arguments, then an object that can refit what it uploaded.  The object
 * keeps on the device the triangles' vertex indices with their slots (16 B a triangle) and a refit schedule (8 B
 * a reached node, plus the offsets of the heights one block walks), and on the host what it needs to find the
 * context's arrays.  It is valid until the next upload on ctx (srt_upload_scene, srt_upload_scene_obj or these
 * calls) or the context's destruction; using it afterwards is the caller's error, and while the context lives
 * srt_scene_refit answers it with SRT_ERR_STATE.  On failure *out is NULL; when the upload itself succeeded the
 * scene stays uploaded.  SRT_ERR_STATE: the layout recomputed for the object disagrees with the context's. */
int srt_upload_scene_refit(srt_context* ctx, const srt_bvh_record* bvhs, uint32_t n_bvhs, const srt_bvh_node* nodes,
                           uint32_t n_nodes, const srt_material_obj* mats, const float* tex_albedo, uint32_t n_mats,
                           const srt_triangle* tris, uint32_t n_tris, const srt_vertex* verts, uint32_t n_verts,
                           struct srt_scene_refit** out);
int srt_upload_scene_obj_refit(srt_context* ctx, const srt_scene* s, struct srt_scene_refit** out);
int srt_scene_refit_destroy(struct srt_scene_refit* r);                   /* NULL: SRT_ERR_INVALID */

#define SRT_SCENE_REFIT_READ_ROOTS 1u

/* Refits the context's device scene to verts_dev: a DEVICE array of n_verts 32-B srt_vertex records, 16-B
 * aligned, on the context's device (the kernels read the first 16 B of each).  Afterwards the node array, its
 * treelet copy where one exists, and the triangle array equal, in every dword, what srt_upload_scene uploads for
 * the nodes srt_bvh_refit yields with these vertices: only the boxes' xyz and the triangles' v0, e1, e2 change;
 * child and triangle slots, counts, flags, treelet ids, materials, input indices, pads and gaps keep their
 * values; the uvs, the materials and the BVH records are not touched.
 *
 * Ordering: the call waits for the context's pipelined sample launches in flight, as every scene mutator does,
 * enqueues its kernels on srt_stream(ctx), and makes every stream the context launches on wait for them, so no
 * later launch reads a half-refit tree.  verts_dev must be ready with respect to srt_stream(ctx) -- written on
 * that stream, or on one it has been made to wait for -- and stay valid until that work has run.
 * flags == 0: only enqueues -- no wait for its own kernels, no allocation, no host copy.  One exception: the
 * streams of the pipelined launches are created by the context's first such launch, and until they exist there
 * is nothing to make wait, so a refit before that launch waits for its own kernels.  Tile culling, which
 * reads host copies of the records' root boxes, stays off until the next upload or a refit with the flag (it
 * only skips provably-sky tiles: the images are the same).
 * SRT_SCENE_REFIT_READ_ROOTS: also synchronises, reads each record's root box back (32 B a record) and keeps
 * tile culling on.
 * The device cannot check the vertices: non-finite positions are the caller's contract.
 * SRT_ERR_INVALID, with the state unchanged and nothing enqueued: a NULL object, a NULL or misaligned
 * verts_dev, n_verts different from the count at upload, unknown flag bits.  SRT_ERR_STATE, likewise: the
 * context's scene arrays are no longer the ones the object was made for. */
int srt_scene_refit(struct srt_scene_refit* r, const srt_vertex* verts_dev, uint32_t n_verts, uint32_t flags);

/* "refit.launches" (kernel launches of one refit), "refit.heights" (heights of the schedule), "refit.count"
 * (refits enqueued so far), "refit.bytes" (device bytes of the index records and the schedule; INT_MAX past it),
 * "refit.treelets" (1: the treelet copy of the node array is written too).  Else SRT_ERR_NOT_FOUND. */
int srt_scene_refit_get_int(struct srt_scene_refit* r, const char* name, int* v);

/* Test and debug readback of ANY context's device scene: waits for the context's work, then copies the node
 * array, its treelet copy and the triangle array to HOST buffers of srt_scene_device_bytes' sizes.  NULL skips
 * an array; the treelet copy is skipped when there is none. */
int srt_scene_copy_device(srt_context* ctx, void* nodes, void* nodes_t, void* tris);
int srt_scene_device_bytes(srt_context* ctx, size_t bytes[3]);     /* nodes, nodes_t (0: none), tris */

#ifdef __cplusplus
}
#endif
#endif
