/*
 * srt_query.h -- device-resident batched ray queries: closest hit and occlusion.
 *
 * A query object owns a device copy of a scene (built from the same std430
 * arrays srt_upload_scene takes) and traces caller-owned device arrays of rays
 * on a caller-owned HIP stream: no host round trip, no allocation and no
 * synchronisation per call.  The semantics are the shader's Intersects loop
 * (ray_intersects.glsl:135-161) under the library's arithmetic contract, so
 * every field is bit-identical to the CPU oracle's oracle_trace_closest.
 *
 * Additive to srt_amd.h (SRT_ABI_VERSION is unchanged); versioned on its own.
 */
#ifndef SRT_QUERY_H
#define SRT_QUERY_H

#include "srt_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SRT_QUERY_ABI_VERSION 1
#define SRT_QUERY_MISS 0xFFFFFFFFu

typedef struct srt_query srt_query;
typedef struct {            /* 32 B */
  uint32_t triangle;        /* flattened (BVH-order) triangle index, as srt_trace_closest reports; 0xFFFFFFFF = miss */
  float    t;               /* final intersection_distance (the input value on a miss) */
  float    normal[3];       /* rec.normal of the hit triangle in the hit BVH's frame (zeros on a miss) */
  uint32_t material;        /* srt_triangle.material_idx of the hit (0 on a miss) */
  uint32_t bvh;             /* index of the BVH record whose traversal produced the final hit (0 on a miss) */
  uint32_t pad;
} srt_hit;

int srt_query_abi_version(void);                                   /* 1 */
/* The scene arrays are validated first, on the host, as srt_upload_scene validates them (SRT_ERR_INVALID:
 * a BVH root, child or triangle index out of range, a cycle, a leaf count >= 2^31), then re-laid and
 * uploaded to `device`.  `stream` is a hipStream_t (NULL = the object creates its own). */
int srt_query_create(int device, void* stream,
                     const srt_bvh_record* bvhs, uint32_t n_bvhs, const srt_bvh_node* nodes, uint32_t n_nodes,
                     const srt_triangle* tris, uint32_t n_tris, const srt_vertex* verts, uint32_t n_verts,
                     srt_query** out);
int srt_query_create_obj(int device, void* stream, const srt_scene* s, srt_query** out);   /* via srt_scene_sizes/_copy */
int srt_query_destroy(srt_query* q);
/* The bvh_count uniform (default n_bvhs); records past n_bvhs read as zeros, as the shader's ghost bvhs[]. */
int srt_query_set_bvh_count(srt_query* q, uint32_t bvh_count);
/* AssetUtils::UpdateModelMatrix; ordered with the queries on the object's stream. */
int srt_query_update_model_matrix(srt_query* q, uint32_t index, const float frame[16]);
/* rays_dev / hits_dev / occluded_dev are DEVICE pointers on the query's device (rays and hits 16-B
 * aligned).  Both calls only enqueue on the query's stream: no allocation on the hot path (scratch is
 * cached in the object and grown when n grows), no synchronisation, no host copy.  n == 0 is SRT_OK and
 * launches nothing.  occluded[i] = 1 iff some triangle is accepted (the walk stops at the first). */
int srt_query_closest(srt_query* q, const srt_ray* rays_dev, uint32_t n, srt_hit* hits_dev);
int srt_query_occluded(srt_query* q, const srt_ray* rays_dev, uint32_t n, uint8_t* occluded_dev);
/* "stack.entries" (tree depth + 1), "stack.in_hbm" (1: the traversal stacks do not fit LDS), "stack.packed"
 * (1: 2-dword entries), "launch.blocks" / "launch.block" (blocks and lanes per block of the last launch),
 * "scratch.bytes" (device scratch the object holds now), "refill.min" (lanes under which a wave refills),
 * "bvh_count"; srt_refit.h adds "refit*" and "layout.*".  SRT_ERR_NOT_FOUND for other names. */
int srt_query_get_int(srt_query* q, const char* name, int* v);
void* srt_query_stream(srt_query* q);

#ifdef __cplusplus
}
#endif
#endif
