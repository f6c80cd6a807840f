/*
 * srt_surface.h -- surface attributes of query hits (albedo, barycentrics, uv) and albedo-demodulated denoising.
 *
 * A surface object owns device copies of what TriangleToSupportedMat reads (raytrace_utils.glsl:140-167): the
 * BVH records' frames, per triangle v0, v1 - v0, v2 - v0, the material index and the three uvs, per material
 * its diffuse colour, use_texture, handle and the optional constant tex_albedo, and the textures as RGBA8.
 * srt_surface_shade turns the srt_hit records srt_query_closest wrote, with the rays that produced them, into
 * one 32-B srt_surface_attr per ray, on the device.  srt_denoise_run_albedo is srt_denoise_run on radiance
 * divided by that albedo (the filter then never blurs the texture) and multiplied back in its last pass.
 *
 * The arithmetic is the library's contract (fp32, source order, no contraction, correctly rounded division;
 * DESIGN.md section 5, "Surface attributes and demodulation"): a float32 restatement reproduces every field
 * bit for bit.
 *
 * Additive to srt_amd.h, srt_query.h and srt_denoise.h (their versions are unchanged); versioned on its own.
 */
#ifndef SRT_SURFACE_H
#define SRT_SURFACE_H

#include "srt_denoise.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SRT_SURFACE_ABI_VERSION 1

typedef struct srt_surface srt_surface;
typedef struct {            /* 32 B */
  float    albedo[3];       /* diffuse, the material's tex_albedo, or the bilinear sample of its texture at uv */
  float    bary_v;          /* barycentric weight of v1 */
  float    bary_w;          /* barycentric weight of v2 (v0's is 1 - v - w) */
  float    uv[2];           /* (u * uv0 + v * uv1) + w * uv2 */
  uint32_t hit;             /* 1 on a hit; on a miss every field of the record is zero */
} srt_surface_attr;

int srt_surface_abi_version(void);                                 /* 1 */
/* The arrays are those srt_upload_scene takes.  They are validated first, on the host, before any device is
 * touched: SRT_ERR_INVALID for a NULL array with a non-zero count, n_bvhs == 0, or a triangle whose vertex or
 * material index is out of range.  tex_albedo (3 floats per material, or NULL) has srt_upload_scene's meaning:
 * when given, use_texture materials take their albedo from it; when NULL they sample texture `handle`
 * (srt_surface_upload_textures) at the hit's uv, and an unknown handle gives zero.  `stream` is a hipStream_t
 * (NULL = the object creates its own). */
int srt_surface_create(int device, void* stream,
                       const srt_bvh_record* bvhs, uint32_t n_bvhs,
                       const srt_material_obj* mats, const float* tex_albedo, uint32_t n_mats,
                       const srt_triangle* tris, uint32_t n_tris,
                       const srt_vertex* verts, uint32_t n_verts,
                       srt_surface** out);
/* srt_upload_scene_obj's rule: with sample_textures it uploads the scene's textures and passes no tex_albedo. */
int srt_surface_create_obj(int device, void* stream, const srt_scene* scene, srt_surface** out);
/* srt_upload_textures' contract: texture i gets handle i, the set replaces any previous one; level 0, GL_LINEAR,
 * GL_REPEAT, texels c / 255; GL_RED reads (r, 0, 0), a 2-channel texture (r, g, 0).  Validated on the host first
 * (SRT_ERR_INVALID: a NULL texel pointer, a size < 1, channels outside 1..4; SRT_ERR_LIMIT: 2^32 texels or more).
 * Waits for the object's stream. */
int srt_surface_upload_textures(srt_surface* s, const srt_texture* textures, uint32_t n);
/* AssetUtils::UpdateModelMatrix; ordered with the shade calls on the object's stream. */
int srt_surface_update_model_matrix(srt_surface* s, uint32_t index, const float frame[16]);
/* The bvh_count uniform (default n_bvhs): a hit whose bvh is at or past it reads a zero frame. */
int srt_surface_set_bvh_count(srt_surface* s, uint32_t bvh_count);
int srt_surface_destroy(srt_surface* s);
void* srt_surface_stream(srt_surface* s);
/* "launch.blocks" / "launch.block" (blocks and lanes per block of the last launch), "textures", "bvh_count".
 * SRT_ERR_NOT_FOUND for other names. */
int srt_surface_get_int(srt_surface* s, const char* name, int* v);
/* rays_dev, hits_dev, attrs_dev: DEVICE arrays of n records on the object's device, 16-B aligned; hits_dev[i] is
 * srt_query_closest's record of rays_dev[i].  Only enqueues one launch on the object's stream: no allocation, no
 * synchronisation, no host copy.  n == 0 is SRT_OK and launches nothing.
 *   miss (triangle == SRT_QUERY_MISS, or a triangle index past the scene's): the whole record is zero;
 *   hit:  b = hits[i].bvh (a record at or past bvh_count, or past n_bvhs, reads as zeros),
 *         mp = (t * xform(frame_b, d, 0)) + xform(frame_b, o, 1), v0p = mp - v0, and with e1 = v1 - v0, e2 = v2 - v0
 *         d00 = dot(e1, e1), d01 = dot(e1, e2), d11 = dot(e2, e2), d20 = dot(v0p, e1), d21 = dot(v0p, e2)
 *         (dot = fma(z, z', fma(y, y', x * x'))), denom = 1.0f / (d00 * d11 - d01 * d01),
 *         v = (d11 * d20 - d01 * d21) * denom, w = (d00 * d21 - d01 * d20) * denom, u = 1 - v - w,
 *         uv = (u * uv0 + v * uv1) + w * uv2; bary_v, bary_w and uv are written for every material. */
int srt_surface_shade(srt_surface* s, const srt_ray* rays_dev, const srt_hit* hits_dev, uint32_t n,
                      srt_surface_attr* attrs_dev);

/* srt_denoise_run with the denoiser's current srt_denoise_params on demodulated radiance.  For a hit pixel p
 * (guide_dev[p].triangle != SRT_QUERY_MISS) with a = max(attrs_dev[p].albedo, albedo_floor) per channel (the floor
 * where the albedo is not greater), the first pass takes C0 = (accum.xyz / float(frames)) / a -- two correctly
 * rounded divisions -- every pass and its colour weight work on these values, and the last pass writes C * a to
 * out_rgba32f_dev and encodes that product to out_rgba8_dev.  Miss pixels pass through as in srt_denoise_run.
 * With passes == 0, attrs_dev is ignored and the result is srt_denoise_run's.  The first and the last pass read
 * attrs_dev directly: the same launches as srt_denoise_run, no buffer of the denoiser's own.
 * SRT_ERR_INVALID (state unchanged): attrs_dev NULL with passes > 0 or not 16-B aligned, albedo_floor not finite
 * or not > 0, and every case in which srt_denoise_run returns it. */
int srt_denoise_run_albedo(srt_denoiser* dn, const void* accum_rgba32f_dev, int frames, const srt_hit* guide_dev,
                           const srt_surface_attr* attrs_dev, float albedo_floor, void* out_rgba32f_dev,
                           void* out_rgba8_dev);

#ifdef __cplusplus
}
#endif
#endif
