/*
 * srt_temporal_motion.h -- temporal reprojection that follows moving models.
 *
 * srt_temporal.h keeps a history for a moving camera over a STATIC scene.  This header adds the other input of
 * the frame loop: UpdateModelMatrix.  The caller states, per BVH record, where the model stands (the record's
 * `frame`, world -> model, and its inverse), and a hit pixel then looks for its surface point where that point
 * was one frame ago:  x_then = model_to_world(then) * world_to_model(now) * x_now.  The guide already carries
 * what is needed: the hit's BVH record, a normal in the record's own (model) frame, which a move does not
 * change, and `t`, which the affine `frame` preserves.
 *
 * Per frame the host makes three calls with the new `frame` of record r:
 *   srt_update_model_matrix(ctx, r, frame);  srt_query_update_model_matrix(q, r, frame);
 *   srt_temporal_set_models(tp, models, n);   -- then renders, queries the guide and calls srt_temporal_accumulate.
 *
 * Definition: an extension of steps 3-4 of srt_temporal.h under the same contract (fp32 in source order, no
 * contraction, correctly rounded division).  The object keeps the poses of the previous accumulated frame (P,
 * n_P of them) and the current ones (Q, n_Q).  At each srt_temporal_accumulate with a valid history, record r is
 *   STATIC  when r >= min(n_P, n_Q) (so also when srt_temporal_set_models was first called after the previous
 *           frame: n_P is 0 then), or when P[r] and Q[r] are bitwise equal (all 128 bytes);
 *   MOVING  otherwise, with the 3 x 4 affine M_r = P[r].model_to_world o Q[r].world_to_model computed on the host.
 *           With A = P[r].model_to_world, B = Q[r].world_to_model, both column-major (element (row i, column k)
 *           is a[4*k + i]), for i = 0..2 and j = 0..3:
 *             M(i, j) = (A(i,0)*B(0,j) + A(i,1)*B(1,j)) + A(i,2)*B(2,j),   and for j == 3 then  + A(i,3).
 * In the kernel a hit pixel of a MOVING record replaces x = t*d + o of step 3 by x' = M_r x:
 *             x'_i = ((M(i,0)*x.x + M(i,1)*x.y) + M(i,2)*x.z) + M(i,3),
 * and everything after it (v = x' - o' onward) is unchanged.  A STATIC record, a record >= n_Q and every pixel of
 * an object without poses take the expression of srt_temporal.h untouched, so an object whose poses never change
 * is bit-identical to one that never had poses.  A miss (id all ones) is tested before anything indexes the
 * poses.  After the call Q becomes P.  srt_temporal_reset drops the history and P and keeps Q.
 *
 * Not modelled, as in any reprojection: the motion of lights, and the change of a moved model's shading (its
 * highlights and shadows move over it; the history blends them at the rate 1/N).  Per-vertex animation, BVH
 * refit and everything srt_temporal.h lists as out of scope stay out of scope.
 *
 * Additive to srt_temporal.h (its version, functions and structs are unchanged); versioned on its own.
 */
#ifndef SRT_TEMPORAL_MOTION_H
#define SRT_TEMPORAL_MOTION_H

#include "srt_temporal.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SRT_TEMPORAL_MOTION_ABI_VERSION 1
#define SRT_TEMPORAL_MAX_MODELS 65535
/* records one upload launch carries in its kernel arguments: "launches" is 1 + ceil(n / 32) while poses are set */
#define SRT_TEMPORAL_MODELS_PER_LAUNCH 32

/* column-major; world_to_model is srt_bvh_record.frame */
typedef struct { float world_to_model[16]; float model_to_world[16]; } srt_temporal_model;

int srt_temporal_motion_abi_version(void);                         /* 1 */
/* The pose of BVH records 0..n-1 for the frames accumulated from now on; it persists until set again.  n == 0
 * (models may then be NULL) returns the object to the static behaviour of srt_temporal.h and to one launch per
 * frame.  The array is read on the host before the call returns.  SRT_ERR_INVALID (state unchanged): a NULL
 * object, NULL models with n > 0, an entry of either matrix that is not finite, a bottom row that is not exactly
 * (0, 0, 0, 1).  SRT_ERR_LIMIT (state unchanged): n > 65535.  The count and the array are checked first, then
 * the object, all before any device is touched.
 * That model_to_world is the inverse of world_to_model is the CALLER's contract: it is not verified.
 * The device memory for the poses (64 B per record) is allocated here and grows only when n exceeds every
 * earlier n, never in srt_temporal_accumulate; srt_temporal_get_int "models.bytes" reports it ("scratch.bytes"
 * does not include it) and "models" reports n.  While n > 0, srt_temporal_accumulate enqueues ceil(n / 32)
 * small upload launches ahead of its kernel (the poses travel in kernel arguments, as the camera does), so it
 * still allocates nothing, never synchronises and makes no host copy. */
int srt_temporal_set_models(srt_temporal* tp, const srt_temporal_model* models, uint32_t n);
/* Convenience: out->world_to_model = frame, out->model_to_world = its affine inverse, computed in double and
 * rounded to float.  SRT_ERR_INVALID: NULL, a non-finite entry, a bottom row that is not (0, 0, 0, 1), a
 * singular 3 x 3 part (determinant 0 or an inverse that is not finite in float). */
int srt_temporal_model_from_frame(const float frame[16], srt_temporal_model* out);

#ifdef __cplusplus
}
#endif
#endif
