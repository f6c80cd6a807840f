/*
 * srt_temporal.h -- temporal reprojection for progressive frames while the camera moves.
 *
 * The interactive loop resets the accumulation on any input, so a moving camera shows 1-spp frames.  A
 * temporal object keeps the previous frame's result and its guide on the device and blends the new frame
 * into the history wherever the same surface point was visible before: a moving 1-spp frame becomes an
 * N-spp one.  The guide is the srt_hit array of the pixel-centre camera rays (srt_denoise_primary_rays +
 * srt_query_closest), the one the denoiser of srt_denoise.h reads; the camera is four plain vectors.
 *
 * Definition ("Temporal reprojection"); fp32 in source order, no contraction, correctly
 * rounded division, dot(a,b) = (a.x*b.x + a.y*b.y) + a.z*b.z.  For pixel p = (i, j):
 *   1. C = accum.xyz / float(frames).
 *   2. No history (the object holds no previous frame, p's guide is a miss, or a check below rejects p):
 *      out = (C, 1.0f).
 *   3. d = the pixel-centre direction of the CURRENT camera as srt_denoise_primary_rays computes it;
 *      x = t*d + o.
 *   4. With o', f', r', u' the PREVIOUS camera: v = x - o'; a = dot(v,f')/dot(f',f'), b = dot(v,r')/dot(r',r'),
 *      c = dot(v,u')/dot(u',u').  Reject unless a > 0.  `a` is the point's distance in the previous frame's t
 *      units when the basis is orthogonal, as UpdateCameraVectors produces it: orthogonality of front, right
 *      and up is a PRECONDITION.
 *   5. uu = (b/a + 0.5)*W - 0.5, vv = (c/a + 0.5)*H - 0.5.  Reject unless uu >= -1 && uu < W && vv >= -1 &&
 *      vv < H (NaN fails).  i0 = floor(uu), j0 = floor(vv), fx = uu - i0, fy = vv - j0.
 *   6. The four taps q = (i0+dx, j0+dy), dy outer, dx inner, weight wb = (dx ? fx : 1-fx) * (dy ? fy : 1-fy).
 *      A tap counts when it lies inside the image, the previous guide at q is a hit with p's BVH record,
 *      dot(n_p, n_q) >= normal_min, |a - t_q| <= depth_tol*(a + t_q), the previous colour at q is finite and
 *      wb > 0.  Over those: sw += wb, sm += wb*C_q, Nh = min(Nh, N_q).
 *   7. If sw > 0: hist = sm/sw, N' = min(Nh + 1, float(max_history)), out = (hist + (1/N')*(C - hist), N');
 *      if C is not finite (and sw > 0): out = (hist, Nh) -- a NaN sample is repaired from the history and not
 *      counted.  Otherwise no history.
 *   8. out and p's guide become the history (a miss keeps id all-ones); the camera becomes the previous one.
 *
 * Composition with the denoiser: out.xyz is a mean, so srt_denoise_run(dn, out, 1, guide, ...) filters it
 * (x / 1.0f is exact); out.w, the history length, is not read by the denoiser.  The denoiser is unchanged.
 *
 * The history assumes a STATIC scene: the caller resets after a scene or model-matrix change.  Only FULL
 * frames are supported (row pitch = width, row 0 at the bottom, index j*W + i), as in srt_denoise.h.  Out of
 * scope: moving geometry and motion vectors, variance estimates, sky (miss) reprojection, band-tiled or
 * multi-GPU frames, sphere scenes.  Models that move between frames: srt_temporal_motion.h, which adds to this
 * header and leaves it as it is.
 *
 * Additive to srt_amd.h, srt_query.h and srt_denoise.h (their versions are unchanged); versioned on its own.
 */
#ifndef SRT_TEMPORAL_H
#define SRT_TEMPORAL_H

#include "srt_query.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SRT_TEMPORAL_ABI_VERSION 1
#define SRT_TEMPORAL_MAX_HISTORY 65535

typedef struct srt_temporal srt_temporal;
typedef struct { float origin[3], front[3], right[3], up[3]; } srt_temporal_camera;
typedef struct {
  uint32_t max_history;  /* 1..65535; blend weight of a new frame never drops below 1/max_history.  Default 32 */
  float    depth_tol;    /* finite, > 0; relative.  Default 0.05 */
  float    normal_min;   /* finite, in [-1, 1]; a tap needs np . nq >= normal_min.  Default 0.9 */
} srt_temporal_params;

int srt_temporal_abi_version(void);                                /* 1 */
/* A temporal object for width x height images on `device`.  `stream` is a hipStream_t (NULL = the object
 * creates its own).  The history (two ping-pong sets of colour | N, normal | t and id per pixel) is allocated
 * here, once.  SRT_ERR_INVALID for a NULL `out` or a dimension < 1, SRT_ERR_LIMIT for an image past 65535 in a
 * dimension or 2^28 pixels (all checked before any device is touched). */
int srt_temporal_create(int device, void* stream, int width, int height, srt_temporal** out);
int srt_temporal_destroy(srt_temporal* tp);
void* srt_temporal_stream(srt_temporal* tp);
/* "width", "height", "max_history", "history" (1 when the object holds a previous frame), "frames" (accumulate
 * calls since the last reset), "scratch.bytes" (device memory the object holds), "launches" (kernels the last
 * call enqueued).  SRT_ERR_NOT_FOUND for other names. */
int srt_temporal_get_int(srt_temporal* tp, const char* name, int* v);
int srt_temporal_get_params(srt_temporal* tp, srt_temporal_params* p);
/* SRT_ERR_INVALID (state unchanged) unless max_history is in 1..65535, depth_tol finite and > 0 and normal_min
 * finite and in [-1, 1]. */
int srt_temporal_set_params(srt_temporal* tp, const srt_temporal_params* p);
/* Drops the history: the next accumulate behaves as the first. */
int srt_temporal_reset(srt_temporal* tp);
/* accum_rgba32f_dev: the accumulation image, a SUM over `frames`.  guide_dev: width * height srt_hit records of
 * the pixel-centre rays of `cam`.  out_rgba32f_dev receives (colour, N).  All are DEVICE pointers, 16-B aligned,
 * and `out` may not alias the inputs; `cam` is read on the host before the call returns.  Only enqueues on the
 * object's stream: one kernel launch, no allocation, no synchronisation, no host copy.
 * SRT_ERR_INVALID: a NULL object, accum, guide, camera or out, frames < 1, a misaligned pointer. */
int srt_temporal_accumulate(srt_temporal* tp, const void* accum_rgba32f_dev, int frames,
                            const srt_hit* guide_dev, const srt_temporal_camera* cam,
                            void* out_rgba32f_dev);

#ifdef __cplusplus
}
#endif
#endif
