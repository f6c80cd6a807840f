/*
 * srt_upsample.h -- guided upsampling of low-resolution progressive frames.
 *
 * A frame's radiance is traced at w x h and reconstructed at W x H = (f * w) x (f * h) with joint-bilateral
 * weights from two closest-hit queries of pixel-centre camera rays (srt_denoise_primary_rays + srt_query_closest
 * at the two sizes): surface edges come from the full-resolution guide, only the lighting is low-resolution.
 * The result is a valid SUM over frames = 1 for srt_temporal_accumulate, srt_denoise_run, _run_albedo and
 * _run_variance.  Camera -> rays -> guides -> upsampled image never leaves the device.
 *
 * The operation ("Guided upsampling"): fp32, source order, no contraction, correctly rounded
 * division; only + - * /, max, abs, comparisons and integer arithmetic, so a float32 restatement reproduces it bit
 * for bit.  Images as in srt_denoise.h: row pitch = width, row 0 at the bottom, index j * W + i.
 *   C[q]  = accum[q].xyz / float(frames);  id(g) = g.bvh's bits on a hit, 0xFFFFFFFF on a miss.
 *   For the full pixel (X, Y) with guide record gP:
 *   n = 2X + 1 - f, i0 = floor(n / 2f), r = n - 2f * i0, a1 = float(r) / float(2f), a0 = 1.0f - a1; the same from Y
 *   gives j0, b0, b1 (the low pixel's centre is the centre of its f x f block of full pixels).
 *   Bilinear stage: taps (i0 + dx, j0 + dy), dy in {0, 1} outer, dx inner, k = a_dx * b_dy.  A tap is skipped when
 *   it lies outside the low image, when id(g_q) != id(gP) or when a component of C[q] is not finite.  For a hit
 *   pixel w = (k * wn) * wz with the denoiser's normal and depth weights between gP and g_q (normal_squarings,
 *   sigma_depth); for a miss pixel w = k.  A tap with !(w > 0) is skipped; sum += w * C[q], sw += w.
 *   If sw > 0 the result is sum / sw.  Otherwise the rescue ring: the 16 taps (i0 - 1 .. i0 + 2) x (j0 - 1 .. j0 + 2),
 *   dy outer, with the same skip rules and w = wn * wz (hit) or 1.0f (miss); sum / sw if sw > 0.  Otherwise the
 *   nearest low pixel C[(Y / f) * w + X / f] as it is, non-finite values included.
 *   out_rgba32f = (result, 1.0f); out_rgba8 its sRGB8 encoding (the context's own), alpha 255.
 * There is no colour weight: there is no full-resolution colour to compare against.
 *
 * Out of scope: non-integer or per-axis factors, sizes that are no multiple of the factor, band-tiled or
 * multi-GPU frames, sphere scenes (they have no mesh to query).
 *
 * Additive to srt_amd.h, srt_query.h and srt_denoise.h (their versions are unchanged); versioned on its own.
 */
#ifndef SRT_UPSAMPLE_H
#define SRT_UPSAMPLE_H

#include "srt_denoise.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SRT_UPSAMPLE_ABI_VERSION 1
#define SRT_UPSAMPLE_MAX_FACTOR 4
#define SRT_UPSAMPLE_LAUNCHES 1  /* kernels one srt_upsample_run enqueues */

typedef struct srt_upsampler srt_upsampler;
typedef struct {
  uint32_t normal_squarings;  /* 0..8, as srt_denoise_params.  Default 5 */
  float    sigma_depth;       /* finite, > 0, as srt_denoise_params.  Default 0.2 */
} srt_upsample_params;

int srt_upsample_abi_version(void);                                /* 1 */
/* An upsampler from low_w x low_h to (factor * low_w) x (factor * low_h) on `device`.  `stream` is a hipStream_t
 * (NULL = the object creates its own).  SRT_ERR_INVALID for a NULL `out`, a factor outside 1..4 or a dimension < 1,
 * SRT_ERR_LIMIT for a FULL size past the denoiser's limits (65535 in a dimension or 2^28 pixels); all checked
 * before any device is touched.  The object holds no device memory. */
int srt_upsample_create(int device, void* stream, int low_w, int low_h, int factor, srt_upsampler** out);
int srt_upsample_destroy(srt_upsampler* up);
void* srt_upsample_stream(srt_upsampler* up);
/* "factor", "low.width", "low.height", "width", "height" (the full size), "launches" (kernels the last run enqueued:
 * 0 before the first, then SRT_UPSAMPLE_LAUNCHES), "scratch.bytes" (device memory the object holds: 0),
 * "launch.blocks" and "launch.block" (the grid of a run: blocks of 32 x 8 full pixels, and lanes per block).
 * SRT_ERR_NOT_FOUND for other names. */
int srt_upsample_get_int(srt_upsampler* up, const char* name, int* v);
int srt_upsample_get_params(srt_upsampler* up, srt_upsample_params* p);
/* SRT_ERR_INVALID (state unchanged) unless normal_squarings <= 8 and sigma_depth is finite and > 0. */
int srt_upsample_set_params(srt_upsampler* up, const srt_upsample_params* p);
/* low_accum_dev: the low-resolution accumulation image (srt_image_pointers), a SUM over `frames`, low_w x low_h,
 * row pitch = low_w.  low_guide_dev: low_w * low_h srt_hit records of the low image's pixel-centre rays;
 * full_guide_dev: width * height records of the full image's.  out_rgba32f_dev receives (result, 1.0f),
 * out_rgba8_dev its sRGB8 encoding with alpha 255; either may be NULL, not both.  All are DEVICE pointers, 16-B
 * aligned (out_rgba8: 4-B), and the outputs may not alias the inputs.  Only enqueues on the object's stream:
 * SRT_UPSAMPLE_LAUNCHES kernel launches, no allocation, no synchronisation, no host copy.
 * SRT_ERR_INVALID (checked before any device is touched): a NULL object, accum or guide, frames < 1, both outputs
 * NULL, a misaligned pointer. */
int srt_upsample_run(srt_upsampler* up, const void* low_accum_dev, int frames, const srt_hit* low_guide_dev,
                     const srt_hit* full_guide_dev, void* out_rgba32f_dev, void* out_rgba8_dev);

#ifdef __cplusplus
}
#endif
#endif
