// temporal.hpp -- the kernel of the temporal reprojection (include/srt_temporal.h; DESIGN.md section 5,
// "Temporal reprojection").
//
// One launch per frame.  A pixel reads its accumulation sum (16 B) and its srt_hit (two 16-B words), finds
// where its surface point lay in the previous frame and gathers the 2 x 2 history pixels around that position:
// per tap the colour | N and the normal | t as 16-B words and the id (the hit's BVH record, all ones for a
// miss) as 4 B.  A wave covers 64 contiguous pixels of a row, so the taps of neighbouring lanes are mostly
// neighbouring addresses and nothing is staged in LDS.  The four taps are loaded from addresses clamped into
// the image before any of them is tested, so the twelve loads are in flight together; a clamped tap is
// rejected by its `inside` flag.  A pure gather: no atomics, and it writes the other set of the ping-pong
// history than the one it reads.
// The arithmetic is the contract's (fp32, source order, no contraction, correctly rounded division).  The 16-B
// loads, the hit unpacking, the luminance and the pixel-centre ray are image_device.hpp's, shared with denoise.hpp.
//
// Moving models (include/srt_temporal_motion.h): the body is a template with two kernels over it.
// temporal_accumulate_kernel is the static instance, the code an object without poses has always run.
// temporal_accumulate_motion_kernel also reads the hit record's 64-B MotionRecord (four 16-B words, one address
// per lane, mostly the same one across a wave) ahead of the taps and moves the surface point by M_r when the
// record is flagged MOVING.  temporal_motion_upload_kernel writes a chunk of those records, which it receives
// by value in its kernel arguments, with ordinary vector stores.
//
// Luminance moments (include/srt_variance.h): a second template parameter adds, to either instance, the moment
// history (m1, m2) as one 8-B word per pixel.  The four extra tap loads are issued with the twelve, ahead of the
// single wait ladder, and accumulate with the colour's weights; the two instances without moments are the code
// they were (the additions are all under `if constexpr`).
//
// Deforming meshes (include/srt_temporal_deform.h): a third template parameter adds, to the two motion instances,
// the triangle's index triple and its three positions in V (the caller's vertices) and in V' (the object's copy of
// the previous frame's), and moves a pixel whose triangle changed to the same barycentric point at the previous
// positions.  The whole addition is one `if constexpr (DEFORM)` block; the four kernels without it are the code
// they were.  temporal_copy_positions_kernel makes V' of V behind the kernel; temporal_deform_upload_kernel
// writes the 96-B DeformRecords as temporal_motion_upload_kernel writes the MotionRecords.
#pragma once

#include "image_device.hpp"
#include "temporal_host.hpp"

namespace srt {
namespace temporal {
using namespace image;

struct TParams {
  const float4* accum;   // the accumulation image (sum | 1)
  const uint4* hits;     // the srt_hit records, 2 uint4 each
  const float4* pcol;    // previous frame: colour | N
  const float4* pgd;     //                 normal | t
  const uint32_t* pid;   //                 id
  float4* ncol;          // this frame's, for the next call
  float4* ngd;
  uint32_t* nid;
  float4* out;           // (colour, N)
  int W, H;
  int has_prev;          // 0: no previous frame, every pixel takes (C, 1)
  float frames;          // float(frames)
  float max_history, depth_tol, normal_min;
  float o[3], p00[3], du[3], dv[3];   // the current camera's pixel-centre basis (denoise_host.hpp PrimaryBasis)
  float po[3], pf[3], pr[3], pu[3];   // the previous camera: origin, front, right, up
};

__device__ __forceinline__ float dot3(float ax, float ay, float az, float bx, float by, float bz) {
  return (ax * bx + ay * by) + az * bz;
}

// A whole 8-B word in one dwordx2, as image_device.hpp's ld16.
typedef float v2f __attribute__((ext_vector_type(2)));
__device__ __forceinline__ float2 ld8(const float2* p) {
  v2f v = *reinterpret_cast<const v2f*>(p);
  asm("" : "+v"(v));
  return make_float2(v.x, v.y);
}

// The moment history of include/srt_variance.h, next to TParams (whose layout the kernels without moments keep).
struct MParams {
  const float2* pm;  // previous frame: m1 | m2
  float2* nm;        // this frame's, for the next call
  float4* out;       // (m1, m2, v, N)
  int has_prev;      // 0: set `pm` holds no moments of the previous frame
};

// The deforming mesh of include/srt_temporal_deform.h, next to TParams and MParams (whose layouts stay).
struct DParams {
  const uint4* tris;     // v0, v1, v2, material per triangle
  const float4* verts;   // V: 2 float4 per srt_vertex, the first holds the position
  const float4* vprev;   // V': 1 float4 per vertex
  const uint4* recs;     // 6 uint4 per BVH record (DeformRecord), n_motion of them; not read when n_motion == 0
  uint32_t n_tris, n_verts;
  int has_vprev;         // 0: every pixel is RIGID (V' holds nothing, or there is no history)
};

// Position `i` of V (stride 2 words) or V' (stride 1): the first 16 B of the record from an index clamped into the
// array; the caller zeroes what an index past the array read.
__device__ __forceinline__ float4 ld_pos(const float4* a, uint32_t i, uint32_t n, uint32_t stride) {
  return ld16(a + (size_t)stride * (i < n ? i : 0u));
}

template <bool MOTION, bool MOMENTS, bool DEFORM = false>
__device__ __forceinline__ void accumulate_pixel(const TParams tp, const uint4* __restrict__ motion, uint32_t n_motion,
                                                 const MParams mp, const DParams dp = DParams()) {
  static_assert(MOTION || !DEFORM, "a deform instance is a motion instance");
  const int i = (int)blockIdx.x * kRowW + ((int)threadIdx.x & (kRowW - 1));
  const int j = (int)blockIdx.y * kRowH + (int)threadIdx.x / kRowW;
  if (i >= tp.W || j >= tp.H) return;
  const int pi = j * tp.W + i;
  const float4 acc = ld16(tp.accum + pi);
  const uint4 h0 = ld16(tp.hits + 2 * (size_t)pi), h1 = ld16(tp.hits + 2 * (size_t)pi + 1);  // triangle t n.x n.y | n.z material bvh pad
  const float cx = acc.x / tp.frames, cy = acc.y / tp.frames, cz = acc.z / tp.frames;
  const uint32_t id = hit_id(h0, h1);
  const float4 g0 = hit_guide(h0, h1);
  const float t = g0.w, nx = g0.x, ny = g0.y, nz = g0.z;
  float4 res = make_float4(cx, cy, cz, 1.0f);
  float L = 0.0f, m1 = 0.0f, m2 = 0.0f, Nm = 1.0f;
  if constexpr (MOMENTS) {
    L = lum(cx, cy, cz);
    m1 = L;
    m2 = L * L;
  }
  if (tp.has_prev && id != kMissId) {
    const float fi = (float)i, fj = (float)j;
    const float dx = pixel_dir(tp.p00[0], tp.du[0], tp.dv[0], tp.o[0], fi, fj);
    const float dy = pixel_dir(tp.p00[1], tp.du[1], tp.dv[1], tp.o[1], fi, fj);
    const float dz = pixel_dir(tp.p00[2], tp.du[2], tp.dv[2], tp.o[2], fi, fj);
    float vx, vy, vz;
    if constexpr (DEFORM) {
      float x = t * dx + tp.o[0], y = t * dy + tp.o[1], z = t * dz + tp.o[2];
      const bool posed = id < n_motion;  // without poses `motion` and `dp.recs` are not read
      // The loads first: the record's ten words, the triangle's indices, then the six positions behind them.
      uint4 r0 = make_uint4(0u, 0u, 0u, 0u), r1 = r0, r2 = r0, r3 = r0, w0 = r0, w1 = r0, w2 = r0, a0 = r0, a1 = r0, a2 = r0;
      if (posed) {
        const uint4* rec = motion + 4 * (size_t)id;
        const uint4* drec = dp.recs + 6 * (size_t)id;
        r0 = ld16(rec), r1 = ld16(rec + 1), r2 = ld16(rec + 2), r3 = ld16(rec + 3);
        w0 = ld16(drec), w1 = ld16(drec + 1), w2 = ld16(drec + 2);
        a0 = ld16(drec + 3), a1 = ld16(drec + 4), a2 = ld16(drec + 5);
      }
      bool deforming = false;
      if (dp.has_vprev) {  // (uniform)
        const uint32_t k = h0.x;  // a hit's triangle; past the mesh: RIGID, and triangle 0 is loaded and not used
        const bool in_mesh = k < dp.n_tris;
        const uint4 idx = ld16(dp.tris + (in_mesh ? k : 0u));
        float4 p0 = ld_pos(dp.verts, idx.x, dp.n_verts, 2u), p1 = ld_pos(dp.verts, idx.y, dp.n_verts, 2u),
               p2 = ld_pos(dp.verts, idx.z, dp.n_verts, 2u);
        float4 q0 = ld_pos(dp.vprev, idx.x, dp.n_verts, 1u), q1 = ld_pos(dp.vprev, idx.y, dp.n_verts, 1u),
               q2 = ld_pos(dp.vprev, idx.z, dp.n_verts, 1u);
        const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (idx.x >= dp.n_verts) p0 = q0 = zero;  // the refit's rule for an index past the array
        if (idx.y >= dp.n_verts) p1 = q1 = zero;
        if (idx.z >= dp.n_verts) p2 = q2 = zero;
        const bool same = __float_as_uint(p0.x) == __float_as_uint(q0.x) && __float_as_uint(p0.y) == __float_as_uint(q0.y) &&
                          __float_as_uint(p0.z) == __float_as_uint(q0.z) && __float_as_uint(p1.x) == __float_as_uint(q1.x) &&
                          __float_as_uint(p1.y) == __float_as_uint(q1.y) && __float_as_uint(p1.z) == __float_as_uint(q1.z) &&
                          __float_as_uint(p2.x) == __float_as_uint(q2.x) && __float_as_uint(p2.y) == __float_as_uint(q2.y) &&
                          __float_as_uint(p2.z) == __float_as_uint(q2.z);
        if (in_mesh && !same) {  // DEFORMING: the same barycentric point of the triangle as it stood in V'
          deforming = true;
          float xm = x, ym = y, zm = z;
          if (posed) {
            xm = ((__uint_as_float(w0.x) * x + __uint_as_float(w0.y) * y) + __uint_as_float(w0.z) * z) + __uint_as_float(w0.w);
            ym = ((__uint_as_float(w1.x) * x + __uint_as_float(w1.y) * y) + __uint_as_float(w1.z) * z) + __uint_as_float(w1.w);
            zm = ((__uint_as_float(w2.x) * x + __uint_as_float(w2.y) * y) + __uint_as_float(w2.z) * z) + __uint_as_float(w2.w);
          }
          const float e1x = p1.x - p0.x, e1y = p1.y - p0.y, e1z = p1.z - p0.z;
          const float e2x = p2.x - p0.x, e2y = p2.y - p0.y, e2z = p2.z - p0.z;
          const float px = xm - p0.x, py = ym - p0.y, pz = zm - p0.z;
          const float d00 = dot3(e1x, e1y, e1z, e1x, e1y, e1z), d01 = dot3(e1x, e1y, e1z, e2x, e2y, e2z);
          const float d11 = dot3(e2x, e2y, e2z, e2x, e2y, e2z);
          const float d20 = dot3(px, py, pz, e1x, e1y, e1z), d21 = dot3(px, py, pz, e2x, e2y, e2z);
          const float denom = 1.0f / (d00 * d11 - d01 * d01);
          const float bv = (d11 * d20 - d01 * d21) * denom;
          const float bw = (d00 * d21 - d01 * d20) * denom;
          const float bu = (1.0f - bv) - bw;
          const float yx = (bu * q0.x + bv * q1.x) + bw * q2.x;
          const float yy = (bu * q0.y + bv * q1.y) + bw * q2.y;
          const float yz = (bu * q0.z + bv * q1.z) + bw * q2.z;
          x = yx;
          y = yy;
          z = yz;
          if (posed) {
            x = ((__uint_as_float(a0.x) * yx + __uint_as_float(a0.y) * yy) + __uint_as_float(a0.z) * yz) + __uint_as_float(a0.w);
            y = ((__uint_as_float(a1.x) * yx + __uint_as_float(a1.y) * yy) + __uint_as_float(a1.z) * yz) + __uint_as_float(a1.w);
            z = ((__uint_as_float(a2.x) * yx + __uint_as_float(a2.y) * yy) + __uint_as_float(a2.z) * yz) + __uint_as_float(a2.w);
          }
        }
      }
      if (!deforming && posed && r3.x != 0u) {  // RIGID and MOVING: x' = M_r x, as the motion instance
        const float mx = ((__uint_as_float(r0.x) * x + __uint_as_float(r0.y) * y) + __uint_as_float(r0.z) * z) + __uint_as_float(r0.w);
        const float my = ((__uint_as_float(r1.x) * x + __uint_as_float(r1.y) * y) + __uint_as_float(r1.z) * z) + __uint_as_float(r1.w);
        const float mz = ((__uint_as_float(r2.x) * x + __uint_as_float(r2.y) * y) + __uint_as_float(r2.z) * z) + __uint_as_float(r2.w);
        x = mx;
        y = my;
        z = mz;
      }
      vx = x - tp.po[0];
      vy = y - tp.po[1];
      vz = z - tp.po[2];
    } else if constexpr (MOTION) {
      float x = t * dx + tp.o[0], y = t * dy + tp.o[1], z = t * dz + tp.o[2];
      // id is a hit's record here (the miss id was tested above); a record past the poses is STATIC
      const bool posed = id < n_motion;
      // One address per lane, whole 16-B words.  Fetching the record once per wave when its lanes share it (a
      // compare against the first lane's id) was measured and is no faster ("Moving models").
      const uint4* rec = motion + 4 * (size_t)(posed ? id : 0u);
      const uint4 r0 = ld16(rec), r1 = ld16(rec + 1), r2 = ld16(rec + 2), r3 = ld16(rec + 3);
      if (posed && r3.x != 0u) {  // MOVING: x' = M_r x, each row as traversal.hpp's xform orders it
        const float mx = ((__uint_as_float(r0.x) * x + __uint_as_float(r0.y) * y) + __uint_as_float(r0.z) * z) + __uint_as_float(r0.w);
        const float my = ((__uint_as_float(r1.x) * x + __uint_as_float(r1.y) * y) + __uint_as_float(r1.z) * z) + __uint_as_float(r1.w);
        const float mz = ((__uint_as_float(r2.x) * x + __uint_as_float(r2.y) * y) + __uint_as_float(r2.z) * z) + __uint_as_float(r2.w);
        x = mx;
        y = my;
        z = mz;
      }
      vx = x - tp.po[0];
      vy = y - tp.po[1];
      vz = z - tp.po[2];
    } else {
      vx = (t * dx + tp.o[0]) - tp.po[0];
      vy = (t * dy + tp.o[1]) - tp.po[1];
      vz = (t * dz + tp.o[2]) - tp.po[2];
    }
    const float a = dot3(vx, vy, vz, tp.pf[0], tp.pf[1], tp.pf[2]) / dot3(tp.pf[0], tp.pf[1], tp.pf[2], tp.pf[0], tp.pf[1], tp.pf[2]);
    const float b = dot3(vx, vy, vz, tp.pr[0], tp.pr[1], tp.pr[2]) / dot3(tp.pr[0], tp.pr[1], tp.pr[2], tp.pr[0], tp.pr[1], tp.pr[2]);
    const float c = dot3(vx, vy, vz, tp.pu[0], tp.pu[1], tp.pu[2]) / dot3(tp.pu[0], tp.pu[1], tp.pu[2], tp.pu[0], tp.pu[1], tp.pu[2]);
    if (a > 0.0f) {
      const float Wf = (float)tp.W, Hf = (float)tp.H;
      const float uu = (b / a + 0.5f) * Wf - 0.5f, vv = (c / a + 0.5f) * Hf - 0.5f;
      if (uu >= -1.0f && uu < Wf && vv >= -1.0f && vv < Hf) {  // NaN fails; only now to integers
        const float fu = __builtin_floorf(uu), fv = __builtin_floorf(vv);
        const int i0 = (int)fu, j0 = (int)fv;  // -1 .. W-1, -1 .. H-1
        const float fx = uu - fu, fy = vv - fv;
        // all twelve loads first (sixteen with moments), from addresses clamped into the image
        float4 qc[4], qg[4];
        float2 qm[4];
        uint32_t qid[4];
        bool inside[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int qx = i0 + (k & 1), qy = j0 + (k >> 1);
          inside[k] = qx >= 0 && qx < tp.W && qy >= 0 && qy < tp.H;
          const int qxc = qx < 0 ? 0 : (qx >= tp.W ? tp.W - 1 : qx), qyc = qy < 0 ? 0 : (qy >= tp.H ? tp.H - 1 : qy);
          const int qi = qyc * tp.W + qxc;
          qid[k] = tp.pid[qi];
          qg[k] = ld16(tp.pgd + qi);
          qc[k] = ld16(tp.pcol + qi);
          if constexpr (MOMENTS) qm[k] = ld8(mp.pm + qi);
        }
        float sw = 0.0f, smx = 0.0f, smy = 0.0f, smz = 0.0f, Nh = __builtin_inff();
        float s1 = 0.0f, s2 = 0.0f;
#pragma unroll
        for (int k = 0; k < 4; ++k) {  // dy outer, dx inner
          const float wb = ((k & 1) ? fx : 1.0f - fx) * ((k >> 1) ? fy : 1.0f - fy);
          const float4 g = qg[k], q = qc[k];
          bool ok = inside[k] && qid[k] == id;
          ok = ok && dot3(nx, ny, nz, g.x, g.y, g.z) >= tp.normal_min;
          ok = ok && __builtin_fabsf(a - g.w) <= tp.depth_tol * (a + g.w);
          ok = ok && finite1(q.x) && finite1(q.y) && finite1(q.z) && wb > 0.0f;
          if (ok) {
            sw += wb;
            smx += wb * q.x;
            smy += wb * q.y;
            smz += wb * q.z;
            Nh = q.w < Nh ? q.w : Nh;
            if constexpr (MOMENTS) {
              s1 += wb * qm[k].x;
              s2 += wb * qm[k].y;
            }
          }
        }
        if (sw > 0.0f) {
          const float hx = smx / sw, hy = smy / sw, hz = smz / sw;
          if (finite1(cx) && finite1(cy) && finite1(cz)) {
            const float n1 = Nh + 1.0f;
            const float N = n1 < tp.max_history ? n1 : tp.max_history;
            const float k = 1.0f / N;
            res = make_float4(hx + k * (cx - hx), hy + k * (cy - hy), hz + k * (cz - hz), N);
            if constexpr (MOMENTS) {
              if (mp.has_prev) {
                const float h1 = s1 / sw, h2 = s2 / sw;
                m1 = h1 + k * (L - h1);
                m2 = h2 + k * (L * L - h2);
                Nm = N;
              }
            }
          } else {
            res = make_float4(hx, hy, hz, Nh);  // a NaN sample: repaired from the history, not counted
            if constexpr (MOMENTS) {
              if (mp.has_prev) {
                m1 = s1 / sw;
                m2 = s2 / sw;
                Nm = Nh;
              }
            }
          }
        }
      }
    }
  }
  tp.out[pi] = res;
  tp.ncol[pi] = res;
  tp.ngd[pi] = g0;
  tp.nid[pi] = id;
  if constexpr (MOMENTS) {
    const float d = m2 - m1 * m1;
    mp.nm[pi] = make_float2(m1, m2);
    mp.out[pi] = make_float4(m1, m2, d > 0.0f ? d : 0.0f, Nm);  // a NaN difference gives 0
  }
}

__global__ __launch_bounds__(kBlock) void temporal_accumulate_kernel(TParams tp) {
  accumulate_pixel<false, false>(tp, nullptr, 0u, MParams());
}

// `motion`: n_motion >= 1 MotionRecords, 64-B aligned.
__global__ __launch_bounds__(kBlock) void temporal_accumulate_motion_kernel(TParams tp, const uint4* __restrict__ motion,
                                                                            uint32_t n_motion) {
  accumulate_pixel<true, false>(tp, motion, n_motion, MParams());
}

// The same two with the luminance moments of include/srt_variance.h.
__global__ __launch_bounds__(kBlock) void temporal_accumulate_moments_kernel(TParams tp, MParams mp) {
  accumulate_pixel<false, true>(tp, nullptr, 0u, mp);
}

__global__ __launch_bounds__(kBlock) void temporal_accumulate_motion_moments_kernel(TParams tp, MParams mp,
                                                                                    const uint4* __restrict__ motion,
                                                                                    uint32_t n_motion) {
  accumulate_pixel<true, true>(tp, motion, n_motion, mp);
}

// The two deform instances (include/srt_temporal_deform.h): the motion instances with the mesh's gathers.  `motion`
// and `dp.recs` hold n_motion records and are not read when it is 0; dp.tris, dp.verts and dp.vprev hold
// dp.n_tris >= 1, dp.n_verts >= 1 and dp.n_verts entries.
__global__ __launch_bounds__(kBlock) void temporal_accumulate_deform_kernel(TParams tp, DParams dp,
                                                                            const uint4* __restrict__ motion,
                                                                            uint32_t n_motion) {
  accumulate_pixel<true, false, true>(tp, motion, n_motion, MParams(), dp);
}

__global__ __launch_bounds__(kBlock) void temporal_accumulate_deform_moments_kernel(TParams tp, MParams mp, DParams dp,
                                                                                    const uint4* __restrict__ motion,
                                                                                    uint32_t n_motion) {
  accumulate_pixel<true, true, true>(tp, motion, n_motion, mp, dp);
}

// V' = the positions of V: one lane per vertex, one 16-B load and one 16-B vector store.
__global__ __launch_bounds__(kBlock) void temporal_copy_positions_kernel(const float4* __restrict__ verts,
                                                                         float4* __restrict__ vprev, uint32_t n_verts) {
  const uint32_t i = blockIdx.x * (uint32_t)kBlock + threadIdx.x;
  if (i >= n_verts) return;
  const float4 p = ld16(verts + 2 * (size_t)i);
  v4f v = {p.x, p.y, p.z, p.w};
  *reinterpret_cast<v4f*>(vprev + i) = v;
}

// One block of kDeformUploadLanes lanes: lane k stores 16-B word k of the chunk, six words a record, records
// [first, first + count) of `dst` (count <= kUploadChunk; the host has checked first + count against the capacity).
constexpr int kDeformUploadLanes = (int)kUploadChunk * 6;
__global__ __launch_bounds__(kDeformUploadLanes) void temporal_deform_upload_kernel(DeformChunk chunk, uint4* __restrict__ dst,
                                                                                    uint32_t first, uint32_t count) {
  const uint32_t k = threadIdx.x;
  if (k >= count * 6u) return;
  const DeformRecord& r = chunk.r[k / 6u];
  const uint32_t w = k % 6u;
  const float* m = (w < 3u ? r.w2m : r.a) + 4 * (w % 3u);
  dst[6 * (size_t)first + k] = make_uint4(__float_as_uint(m[0]), __float_as_uint(m[1]), __float_as_uint(m[2]), __float_as_uint(m[3]));
}

// One block of kUploadLanes lanes: lane k stores 16-B word k of the chunk, records [first, first + count) of `dst`
// (count <= kUploadChunk; the host has checked first + count against the array's capacity).
constexpr int kUploadLanes = (int)kUploadChunk * 4;
__global__ __launch_bounds__(kUploadLanes) void temporal_motion_upload_kernel(MotionChunk chunk, uint4* __restrict__ dst,
                                                                              uint32_t first, uint32_t count) {
  const uint32_t k = threadIdx.x;
  if (k >= count * 4u) return;
  const MotionRecord& r = chunk.r[k >> 2];
  const uint32_t w = k & 3u;
  const float* m = r.m + 4 * (w < 3u ? w : 0u);
  const uint4 v = w < 3u ? make_uint4(__float_as_uint(m[0]), __float_as_uint(m[1]), __float_as_uint(m[2]), __float_as_uint(m[3]))
                         : make_uint4(r.moving, 0u, 0u, 0u);
  dst[4 * (size_t)first + k] = v;
}

}  // namespace temporal
}  // namespace srt
