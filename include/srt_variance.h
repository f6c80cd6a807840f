/*
 * srt_variance.h -- temporal luminance moments and a variance-guided a-trous filter (the SVGF weights).
 *
 * srt_denoise.h weighs a tap's colour difference against one global sigma_color.  This header gives the filter a
 * per-pixel noise estimate instead: the temporal object integrates the first two moments of the luminance with
 * the taps and weights of its colour history, and the filter scales the luminance difference of a tap by the
 * square root of the (blurred) variance at the pixel.  A pixel with a long, quiet history is barely touched, a
 * freshly disoccluded or noisy one is filtered hard, and the estimate shrinks pass by pass as the filter itself
 * removes variance.  Opt-in: srt_temporal_accumulate and srt_denoise_run compute what they always did.
 *
 * Contract, as in the headers this one adds to: fp32 in source order, no contraction, correctly rounded division,
 * dot(a,b) = (a.x*b.x + a.y*b.y) + a.z*b.z, and ONE addition: a correctly rounded fp32 square root (what numpy's
 * float32 sqrt computes).  No other transcendental.  "finite" is the test of the exponent bits.
 *   lum(c) = (0.2126f*c.x + 0.7152f*c.y) + 0.0722f*c.z
 *
 * 1. Temporal moments (srt_temporal_accumulate_moments).  C, the taps q, wb, sw, Nh and N' are exactly those of
 *    srt_temporal.h steps 1-7 (with srt_temporal_motion.h's x' where poses are set); `out` is bit for bit what
 *    srt_temporal_accumulate writes.  The object keeps (m1, m2) per pixel next to the colour history.  L = lum(C).
 *      a. No history -- step 2 of srt_temporal.h (no previous frame, a miss, a rejected pixel, sw == 0), or the
 *         MOMENT history is invalid (the previous frame was accumulated by srt_temporal_accumulate, or moments
 *         were enabled after it): (m1, m2) = (L, L*L), N = 1.  This holds whatever C is.
 *      b. Otherwise (sw > 0 and a valid moment history): h1 = (sum wb*m1_q)/sw, h2 = (sum wb*m2_q)/sw over the
 *         counted taps in their order; if C is finite  m1 = h1 + (1/N')*(L - h1), m2 = h2 + (1/N')*(L*L - h2),
 *         N = N';  if C is not finite  (m1, m2) = (h1, h2), N = Nh.  A counted tap's moments are taken as they
 *         are (a tap counts by its COLOUR being finite).
 *      c. d = m2 - m1*m1;  v = d > 0 ? d : 0  (a NaN gives 0).
 *    out_moments = (m1, m2, v, N); (m1, m2) become the moment history.  srt_temporal_reset drops both histories.
 *    N of case (b) is the colour history's length even when the moment history is younger (after a plain call).
 *
 * 2. The variance-guided filter (srt_denoise_run_variance): 1 + passes launches.  ids, wn and wz are those of
 *    srt_denoise.h's filter: id = the hit's BVH record, all ones for a miss; wn = max(dot(n_p, n_q), 0) squared
 *    normal_squarings times; xz = |t_p - t_q| / (sigma_depth*(t_p + t_q)), wz = 1/((1 + xz)*(1 + xz)).
 *    Resolve launch:  C_0 = colour.xyz / float(frames);  the guide is packed;  var_0[p] =
 *      0                                   for a miss pixel;
 *      moments[p].z                        for a hit pixel with moments[p].w >= float(min_history);
 *      the spatial estimate                for every other hit pixel (a NaN history length included):
 *        over (dx, dy) in [-3, 3]^2, dy outer, dx inner, a tap q = p + (dx, dy) counts when it lies inside the
 *        image, has p's id and moments[q].x and moments[q].y are both finite; w = wn*wz (no test of w);
 *        s1 += w*m1_q, s2 += w*m2_q, sw += w.  If sw > 0: a = s1/sw, b = s2/sw, d = b - a*a,
 *        var_0 = (d > 0 ? d : 0) * (float(min_history)/moments[p].w); otherwise var_0 = 0.
 *    Pass i = 0 .. passes-1, step s = 2^i, for a hit pixel p:
 *      g: over the 3 x 3 neighbours q' = p + (dx, dy), dx, dy in -1..1 (NOT scaled by s), dy outer, kg = 1/4 at the
 *         centre, 1/8 on the edges, 1/16 at the corners; a neighbour outside the image, with another id or with a
 *         non-finite var_i is skipped; sg += kg*var_i[q'], sk += kg; g = sk > 0 ? sg/sk : 0.
 *      sl = sigma_lum*sqrt(g) + 1e-4f.   Lp = lum(C_i[p]).
 *      The 25 taps q = p + s*(dx, dy), dx, dy in -2..2, dy outer, k = h[|dx|]*h[|dy|], h = (3/8, 1/4, 1/16): a tap
 *         outside the image, with another id or with a non-finite colour is skipped.  xl = |Lp - lum(C_i[q])| / sl,
 *         wl = 1/((1 + xl)*(1 + xl)), and wl = 1 when Lp is not finite.  w = ((k*wn)*wz)*wl; the tap is skipped
 *         unless w > 0.  sw += w, sum += w*C_i[q], sv += (w*w)*var_i[q] (only when var_i[q] is finite).
 *      If sw > 0: C_{i+1}[p] = sum/sw and var_{i+1}[p] = sv/(sw*sw); otherwise both pass through.
 *      A miss pixel passes its colour through with variance 0.  sigma_lum is the same in every pass.
 *    The last pass writes (colour, 1) and / or sRGB8 exactly as srt_denoise_run does, and var_passes to out_var.
 *
 * Out of scope: albedo demodulation (it needs uv from the query service), moments from the tracer's own samples,
 * sky reprojection, band-tiled or multi-GPU frames, sphere scenes, any change to srt_denoise_run's weights.
 *
 * Additive to srt_temporal.h, srt_temporal_motion.h and srt_denoise.h (their versions, functions and structs are
 * unchanged); versioned on its own.
 */
#ifndef SRT_VARIANCE_H
#define SRT_VARIANCE_H

#include "srt_temporal_motion.h"
#include "srt_denoise.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SRT_VARIANCE_ABI_VERSION 1
#define SRT_VARIANCE_MAX_MIN_HISTORY 65535

typedef struct {
  float    sigma_lum;    /* finite, > 0.  Default 1.0 */
  uint32_t min_history;  /* 1..65535; below it the variance is the spatial estimate.  Default 4 */
} srt_denoise_var_params;

int srt_variance_abi_version(void);                                /* 1 */

/* Allocates the moment history: two ping-pong float2 arrays, 16 B per pixel in all.  Idempotent.
 * srt_temporal_get_int "moments.bytes" reports the allocation (0 before); "scratch.bytes" does not count it. */
int srt_temporal_enable_moments(srt_temporal* tp);
/* srt_temporal_accumulate, and out_moments_dev receives one float4 (m1, m2, v, N) per pixel (a DEVICE pointer,
 * 16-B aligned, no alias of the other pointers).  Only enqueues: the launches srt_temporal_accumulate makes, no
 * allocation.  Calls of the two functions may be mixed: a plain srt_temporal_accumulate advances the colour history
 * and leaves the moment history invalid for the next frame (case 1a, for the moments only).
 * SRT_ERR_INVALID: what srt_temporal_accumulate rejects, moments not enabled, out_moments_dev NULL or misaligned. */
int srt_temporal_accumulate_moments(srt_temporal* tp, const void* accum_rgba32f_dev, int frames,
                                    const srt_hit* guide_dev, const srt_temporal_camera* cam,
                                    void* out_rgba32f_dev, void* out_moments_dev);

/* Allocates two ping-pong float variance arrays, 8 B per pixel in all.  Idempotent.  srt_denoise_get_int
 * "variance.bytes" reports the allocation (0 before); "scratch.bytes" does not count it. */
int srt_denoise_enable_variance(srt_denoiser* dn);
int srt_denoise_get_var_params(srt_denoiser* dn, srt_denoise_var_params* p);
/* SRT_ERR_INVALID (state unchanged) unless sigma_lum is finite and > 0 and min_history is in 1..65535. */
int srt_denoise_set_var_params(srt_denoiser* dn, const srt_denoise_var_params* p);
/* colour_rgba32f_dev: a SUM over `frames` (srt_temporal_accumulate_moments' out with frames = 1); guide_dev: the
 * srt_hit records; moments_dev: (m1, m2, v, N) per pixel.  Uses passes, normal_squarings and sigma_depth of
 * srt_denoise_params and ignores sigma_color.  out_rgba32f_dev / out_rgba8_dev as srt_denoise_run (either may be
 * NULL, not both); out_var_f32_dev (may be NULL) receives one float per pixel.  DEVICE pointers, 16-B aligned
 * (out_rgba8 and out_var: 4-B), outputs no alias of the inputs.  Only enqueues 1 + passes launches ("launches").
 * SRT_ERR_INVALID: a NULL object, colour, guide or moments, frames < 1, passes == 0, variance not enabled, both
 * colour outputs NULL, a misaligned pointer. */
int srt_denoise_run_variance(srt_denoiser* dn, const void* colour_rgba32f_dev, int frames, const srt_hit* guide_dev,
                             const void* moments_dev, void* out_rgba32f_dev, void* out_rgba8_dev,
                             void* out_var_f32_dev);

#ifdef __cplusplus
}
#endif
#endif
