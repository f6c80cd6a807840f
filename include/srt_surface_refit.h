/*
 * srt_surface_refit.h -- a surface object that follows a mesh whose vertices move.
 *
 * srt_surface.h's object holds, per triangle, v0, v1 - v0 and v2 - v0 as they were at creation.  With
 * SRT_SURFACE_REFIT the object also keeps the triangles' vertex indices on the device (16 B a triangle), and
 * srt_surface_refit rewrites those three fields from a DEVICE vertex array -- the one srt_query_refit
 * (srt_refit.h) is given -- so the barycentrics and uv of a deformed query's hits need no re-created object.
 * The uvs, materials, frames and textures stay as created.
 *
 * Additive to srt_surface.h (SRT_SURFACE_ABI_VERSION, its structs and functions are unchanged); versioned on its
 * own.
 */
#ifndef SRT_SURFACE_REFIT_H
#define SRT_SURFACE_REFIT_H

#include "srt_surface.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SRT_SURFACE_REFIT_ABI_VERSION 1
#define SRT_SURFACE_REFIT 1u   /* srt_surface_create_ex flag: the object can be refit */

int srt_surface_refit_abi_version(void);                           /* 1 */

/* srt_surface_create / srt_surface_create_obj with flags; flags == 0 is exactly those calls.  An unknown flag
 * bit is SRT_ERR_INVALID, before any device is touched. */
int srt_surface_create_ex(int device, void* stream,
                          const srt_bvh_record* bvhs, uint32_t n_bvhs,
                          const srt_material_obj* mats, const float* tex_albedo, uint32_t n_mats,
                          const srt_triangle* tris, uint32_t n_tris,
                          const srt_vertex* verts, uint32_t n_verts,
                          uint32_t flags, srt_surface** out);
int srt_surface_create_obj_ex(int device, void* stream, const srt_scene* scene, uint32_t flags, srt_surface** out);

/* verts_dev: a DEVICE array of n_verts 32-B srt_vertex records, 16-B aligned, on the object's device (the kernel
 * reads the first 16 B of each).  Enqueues one kernel on the object's stream, ordered with the shade calls there:
 * no allocation, no synchronisation, no host copy; verts_dev must stay valid until that work has run.  The
 * kernel rewrites each triangle's v0, v1 - v0, v2 - v0 (the fp32 subtractions srt_surface_create makes); a vertex
 * index is in range by srt_surface_create's validation.  Afterwards those fields equal, in every dword, what
 * srt_surface_create uploads for the same vertices.
 * SRT_ERR_INVALID, with the state unchanged and nothing enqueued: a NULL object, an object created without
 * SRT_SURFACE_REFIT, a NULL or misaligned verts_dev, n_verts different from the count at creation. */
int srt_surface_refit(srt_surface* s, const srt_vertex* verts_dev, uint32_t n_verts);

/* srt_surface_get_int also answers: "refit" (1: created with SRT_SURFACE_REFIT), "refit.bytes" (device bytes of
 * the vertex indices) and "refit.count" (refits enqueued so far) -- all 0 without the flag. */

#ifdef __cplusplus
}
#endif
#endif
