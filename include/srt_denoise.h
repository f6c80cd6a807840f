/*
 * srt_denoise.h -- an edge-avoiding (a-trous) filter for progressive frames, guided by ray queries.
 *
 * The interactive loop shows 1-8 spp frames.  A denoiser object filters the accumulation image of such a
 * frame on the device, guided by the srt_hit records of one closest-hit query over the pixel-centre camera
 * rays (srt_denoise_primary_rays + srt_query_closest): triangle-or-miss, t, unit normal and BVH record are
 * the G-buffer.  Camera -> rays -> guide -> filtered image never leaves the device.
 *
 * The filter ("Denoiser") is `passes` passes of a 5x5 B3-spline kernel with holes
 * (step 2^i in pass i), each tap weighted by normal, depth and colour similarity; fp32, source order, no
 * contraction, correctly rounded division, no transcendentals: a float32 restatement reproduces it bit for bit.
 *
 * Only FULL frames are supported: the image of a single untiled context (srt_image_pointers) or a group's
 * assembled full-frame image (srt_group_image_pointers), row pitch = width.  Band-tiled (multi-rank)
 * denoising is out of scope: a rank's row bands lack the neighbours the taps read.
 *
 * Additive to srt_amd.h and srt_query.h (their versions are unchanged); versioned on its own.
 */
#ifndef SRT_DENOISE_H
#define SRT_DENOISE_H

#include "srt_query.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SRT_DENOISE_ABI_VERSION 1
#define SRT_DENOISE_MAX_PASSES 8
#define SRT_DENOISE_MAX_NORMAL_SQUARINGS 8

typedef struct srt_denoiser srt_denoiser;
typedef struct {
  uint32_t passes;            /* 0..8; pass i uses step 2^i and sigma_color * 2^-i.  Default 5 */
  uint32_t normal_squarings;  /* 0..8; the normal weight is max(np . nq, 0)^(2^normal_squarings).  Default 5 */
  float    sigma_color;       /* finite, > 0.  Default 3.0 */
  float    sigma_depth;       /* finite, > 0; relative: |tp - tq| / (sigma_depth * (tp + tq)).  Default 0.2 */
} srt_denoise_params;

int srt_denoise_abi_version(void);                                 /* 1 */
/* A denoiser for width x height images on `device`.  `stream` is a hipStream_t (NULL = the object creates
 * its own).  The ping-pong colour buffers and the packed guide are allocated here, once.  SRT_ERR_INVALID for
 * a NULL `out` or a dimension < 1, SRT_ERR_LIMIT for an image past 65535 in a dimension or 2^28 pixels (all
 * checked before any device is touched). */
int srt_denoise_create(int device, void* stream, int width, int height, srt_denoiser** out);
int srt_denoise_destroy(srt_denoiser* dn);
void* srt_denoise_stream(srt_denoiser* dn);
/* "passes", "normal_squarings", "width", "height", "scratch.bytes" (device memory the object holds),
 * "tile.lds_bytes" (LDS of a block of the tiled kernel at its largest step), "tile.max_step" (the largest step
 * that takes the LDS-tiled kernel; larger steps read their taps from global memory; 0: none is tiled),
 * "tile.width" / "tile.height", "launches" (kernels the last run enqueued).  SRT_ERR_NOT_FOUND for other names. */
int srt_denoise_get_int(srt_denoiser* dn, const char* name, int* v);
int srt_denoise_get_params(srt_denoiser* dn, srt_denoise_params* p);
/* SRT_ERR_INVALID (state unchanged) unless passes <= 8, normal_squarings <= 8 and both sigmas finite and > 0. */
int srt_denoise_set_params(srt_denoiser* dn, const srt_denoise_params* p);
/* The width * height pixel-centre camera rays into rays_dev (a DEVICE array, 16-B aligned): index j * width + i,
 * row j = 0 at the bottom, intersection_distance 1e30f, pad0 0.  du = right / W, dv = up / H,
 * p00 = (o + front - right/2 - up/2) + 0.5 * (du + dv), direction = (p00 + i*du + j*dv) - o, in that order,
 * unfused.  Only enqueues on the object's stream. */
int srt_denoise_primary_rays(srt_denoiser* dn, const float origin[3], const float front[3], const float right[3],
                             const float up[3], srt_ray* rays_dev);
/* accum_rgba32f_dev: the accumulation image as srt_image_pointers / srt_group_image_pointers return it, a SUM
 * over `frames`, full frame, row pitch = width.  guide_dev: width * height srt_hit records of the pixel-centre
 * rays (may be NULL when passes == 0).  out_rgba32f_dev receives (filtered colour, 1.0f), out_rgba8_dev that
 * colour through the context's own linear -> sRGB8 encoding with alpha 255 (with passes == 0 bit-identical to
 * the context's image0); either may be NULL, not both.  All are DEVICE pointers, 16-B aligned (out_rgba8: 4-B),
 * and may not alias the inputs.  Only enqueues on the object's stream: `passes` kernel launches (one when
 * passes == 0), no allocation, no synchronisation, no host copy.
 * SRT_ERR_INVALID: a NULL object or accum, frames < 1, a NULL guide with passes > 0, both outputs NULL. */
int srt_denoise_run(srt_denoiser* dn, const void* accum_rgba32f_dev, int frames, const srt_hit* guide_dev,
                    void* out_rgba32f_dev, void* out_rgba8_dev);

#ifdef __cplusplus
}
#endif
#endif
