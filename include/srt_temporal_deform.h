/*
 * srt_temporal_deform.h -- temporal reprojection that follows a mesh whose vertices move.
 *
 * srt_temporal_motion.h follows a model that moves as a whole (its `frame`).  This header adds the third input of
 * an animated frame loop: the vertices themselves, the array srt_query_refit (srt_refit.h) is given.  The object
 * is told the mesh's vertex indices once (srt_temporal_set_mesh) and, per frame, the DEVICE array of the vertices
 * the frame was traced against (srt_temporal_set_vertices).  It keeps a copy of the positions the previous
 * accumulate read, and a hit pixel then looks for its MATERIAL point -- the same barycentric position in the same
 * triangle -- where that point was one frame ago.
 *
 * Per frame, for a deforming mesh, on one stream or with the streams ordered:
 *   srt_query_refit(q, verts_dev, n);  srt_temporal_set_vertices(tp, verts_dev, n);  [srt_surface_refit(s, ...)]
 *   -- then render, query the guide, srt_temporal_accumulate.
 *
 * Definition: an extension of steps 3-4 of srt_temporal.h under the same contract (fp32 in source order, no
 * contraction, correctly rounded division); dot(a, b) = (a.x*b.x + a.y*b.y) + a.z*b.z -- the temporal contract's
 * dot, NOT the fused multiply-adds of srt_surface.h's barycentrics -- and an affine matrix M (3 rows of 4) is
 * applied as  affine(M, x)_i = ((M(i,0)*x.x + M(i,1)*x.y) + M(i,2)*x.z) + M(i,3),  as the MOVING path orders it.
 * A column-major srt_temporal_model matrix a[] has M(i, j) = a[4*j + i].
 *
 * The object keeps V', the positions the previous accumulate read; V is the array set now; P, Q, n_P, n_Q are
 * the poses of srt_temporal_motion.h.  For a hit pixel with BVH record r, hit triangle k = hits[p].triangle and
 * vertex indices (i0, i1, i2) = tris[k] the pixel is
 *   RIGID      if the object holds no history; or V or V' is absent (V' is absent on the first accumulate after
 *              srt_temporal_set_mesh, after srt_temporal_reset and after srt_temporal_set_vertices(NULL)); or
 *              k >= n_tris; or the nine position floats of the three vertices are bitwise equal in V and V'.
 *              A RIGID pixel takes today's expression, STATIC or MOVING as the poses say, unchanged: a mesh whose
 *              vertices do not change is bit-identical to an object without a mesh.
 *   DEFORMING  otherwise.  A vertex index >= n_verts reads (0,0,0) in both arrays (the refit's rule; the load is
 *              guarded, nothing is read past either array).  Then
 *     1. x = t*d + o;  xm = affine(Q[r].world_to_model, x) when r < n_Q, else xm = x.
 *     2. p0, p1, p2 from V;  e1 = p1 - p0, e2 = p2 - p0, v0p = xm - p0;
 *        d00 = dot(e1,e1), d01 = dot(e1,e2), d11 = dot(e2,e2), d20 = dot(v0p,e1), d21 = dot(v0p,e2);
 *        denom = 1.0f / (d00*d11 - d01*d01);
 *        v = (d11*d20 - d01*d21) * denom;  w = (d00*d21 - d01*d20) * denom;  u = (1.0f - v) - w.
 *     3. q0, q1, q2 from V';  per component  ym = (u*q0 + v*q1) + w*q2.
 *     4. x' = affine(A, ym) with A = P[r].model_to_world when r < min(n_P, n_Q), A = Q[r].model_to_world when
 *        n_P <= r < n_Q, and x' = ym when r >= n_Q.
 *     5. everything from v = x' - o' onward is unchanged.  A degenerate triangle gives a non-finite v / w, which
 *        the existing tests of steps 4-5 reject to "no history"; there is no special case.
 *   Step 6's tap checks are unchanged (same record, normal, depth).
 * After the accumulate kernel, on the same stream, the object copies V's positions into its own V' (one more
 * launch; no allocation, synchronisation or host copy), so the caller may reuse verts_dev once that work has run.
 * After the call Q becomes P, as before.
 *
 * Launches ("launches") of one accumulate while a deform instance runs with n poses set:
 *   1 (the kernel) + ceil(n / 32) (the 64-B motion records) + ceil(n / 32) (the 96-B deform records: the rows of
 *   Q[r].world_to_model and of A) + 1 (the copy of V into V').  Without poses that is one more than today's.
 * A deform instance runs when a mesh is attached and V is set; otherwise the object runs the kernels and enqueues
 * the launches it ran before this header existed.
 *
 * Not modelled: topology changes and a changing n_verts, a history-validity test per triangle beyond step 6,
 * motion of lights, and what srt_temporal_motion.h lists.
 *
 * Additive to srt_temporal.h and srt_temporal_motion.h (their versions, structs and functions are unchanged);
 * versioned on its own.
 */
#ifndef SRT_TEMPORAL_DEFORM_H
#define SRT_TEMPORAL_DEFORM_H

#include "srt_temporal_motion.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SRT_TEMPORAL_DEFORM_ABI_VERSION 1
#define SRT_TEMPORAL_MAX_MESH (1u << 28)   /* n_tris and n_verts stay below it */

int srt_temporal_deform_abi_version(void);                         /* 1 */

/* Host arrays, read before the call returns.  Uploads the triangles' vertex indices (16 B each) and allocates
 * the object's own copy of the previous positions (16 B a vertex), and, while poses are set, the deform records
 * (96 B a record, grown as "models.bytes" grows): the only allocations of the feature, none of them in
 * srt_temporal_accumulate.  Waits for the object's stream.  V and V' are dropped.  n_tris == 0 (tris may then be
 * NULL) detaches the mesh and returns the object to the behaviour and the launch count it had without one.
 * SRT_ERR_LIMIT: n_tris or n_verts >= 2^28.  SRT_ERR_INVALID: NULL tris with n_tris > 0, n_verts == 0 with
 * n_tris > 0, a NULL object.  The counts are checked first, then the array, then the object, all with the state
 * unchanged and before any device is touched. */
int srt_temporal_set_mesh(srt_temporal* tp, const srt_triangle* tris, uint32_t n_tris, uint32_t n_verts);
/* DEVICE array of n_verts 32-B srt_vertex records, 16-B aligned: the array handed to srt_query_refit for the
 * frame about to be accumulated (the kernels read the first 16 B of each).  It applies to the accumulate calls
 * from now on, until set again; NULL makes every pixel RIGID and drops the previous positions.  It must stay
 * valid until the accumulate work that reads it has run.  Enqueues nothing.
 * SRT_ERR_INVALID (state unchanged): a misaligned pointer, a NULL object, no mesh attached, n_verts different
 * from the mesh's (also with a NULL array). */
int srt_temporal_set_vertices(srt_temporal* tp, const srt_vertex* verts_dev, uint32_t n_verts);

/* srt_temporal_get_int also answers: "mesh.tris", "mesh.verts" (0 without a mesh), "mesh.bytes" (device bytes of
 * the vertex indices, the previous positions and the deform records; no part of "scratch.bytes", as
 * "models.bytes" is none) and "deform" (1 when the last accumulate ran a deform instance). */

#ifdef __cplusplus
}
#endif
#endif
