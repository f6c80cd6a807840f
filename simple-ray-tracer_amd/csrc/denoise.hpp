// denoise.hpp -- the kernels of the edge-avoiding denoiser (include/srt_denoise.h; DESIGN.md section 5,
// "Denoiser").
//
// One launch per pass.  A pixel is two float4: colour | id (id: the BVH record of its hit as bits, all ones
// for a miss or a pixel outside the image) and normal | t, so a tap reads two 16-B words and its whole
// rejection test is one compare of ids.  The first pass reads the accumulation sum and the 32-B srt_hit
// records instead (mean and guide pack fused into its loads) and writes the packed guide for the later
// passes; the last pass writes the outputs (sRGB8 encode fused into its store).
//   denoise_tiled_kernel   small steps: a 32 x 8 tile and its halo of 2 * step pixels staged once in LDS
//                          (linear 16-B loads and ds_write_b128; a wave's tap is 2 rows of 32 contiguous
//                          float4 = every bank once per ds_read_b128 lane group, whatever the row stride)
//   denoise_direct_kernel  large steps, where the halo outgrows the tile: taps are global dwordx4 loads, a
//                          wave covering 64 contiguous pixels of one row
// The arithmetic is the contract's (fp32, source order, no contraction, correctly rounded division).  The 16-B
// loads, the hit unpacking, the normal and depth weights, the luminance and the sRGB8 encode are image_device.hpp's,
// shared with temporal.hpp.
#pragma once

#include "denoise_host.hpp"
#include "image_device.hpp"

namespace srt {
namespace denoise {
using namespace dev;
using namespace image;

struct DParams {
  const float4* src;   // colour | id of the previous pass; first pass: the accumulation image (sum | 1)
  const uint4* hits;   // first pass: the srt_hit records, 2 uint4 each
  float4* guide;       // normal | t: written by the first pass, read by the others
  float4* dst;         // colour | id for the next pass (nullptr in the last pass)
  float4* out32;       // last pass: (colour, 1) or nullptr
  uint32_t* out8;      // last pass: sRGB8 or nullptr
  int W, H, step;
  int nsq;             // normal_squarings
  float frames;        // first pass: float(frames)
  float sigma_c, sigma_d;
};

struct Px {
  float4 c;  // colour | id
  float4 g;  // normal | t
};

// srt_denoise_run_albedo (include/srt_surface.h): the pass kernels instantiated over AParams filter radiance
// divided by the surface albedo.  Their first pass divides the mean of a hit pixel by a = max(albedo, floor) as
// it loads it, their last pass multiplies the filtered colour by a before it stores it; both read the
// srt_surface_attr records directly (albedo | bary_v in the first of a record's two float4).  The instances over
// DParams are the ones srt_denoise_run launches and read none of this.
struct AParams : DParams {
  const float4* attrs;  // 2 float4 per srt_surface_attr
  float floor;          // albedo_floor
};
template <class P>
constexpr bool kAlbedo = false;
template <>
constexpr bool kAlbedo<AParams> = true;

__device__ __forceinline__ f3 albedo_of(const AParams& ap, int p) {
  const float4 a = ap.attrs[2 * (size_t)p];
  return mk(a.x > ap.floor ? a.x : ap.floor, a.y > ap.floor ? a.y : ap.floor, a.z > ap.floor ? a.z : ap.floor);
}

__device__ __forceinline__ uint32_t px_id(const float4& c) { return __float_as_uint(c.w); }
__device__ __forceinline__ bool finite3(const float4& c) { return finite1(c.x) && finite1(c.y) && finite1(c.z); }

template <bool FIRST, class P = DParams>
__device__ __forceinline__ Px load_px(const P& dp, int p) {
  Px r;
  if constexpr (FIRST) {
    const float4 a = ld16(dp.src + p);
    const uint4 h0 = ld16(dp.hits + 2 * (size_t)p), h1 = ld16(dp.hits + 2 * (size_t)p + 1);  // triangle t n.x n.y | n.z material bvh pad
    f3 o = mk(a.x, a.y, a.z) / dp.frames;
    if constexpr (kAlbedo<P>) {
      if (h0.x != kMissId) {
        const f3 al = albedo_of(dp, p);
        o = mk(o.x / al.x, o.y / al.y, o.z / al.z);
      }
    }
    r.c = make_float4(o.x, o.y, o.z, __uint_as_float(hit_id(h0, h1)));
    r.g = hit_guide(h0, h1);
  } else {
    r.c = ld16(dp.src + p);
    r.g = ld16(dp.guide + p);
  }
  return r;
}

// One tap of a pixel whose own id is a hit's.  `k` is the B3-spline weight h[|dx|] * h[|dy|].
__device__ __forceinline__ void tap(const DParams& dp, const Px& p, bool pfin, const float4& cq, const float4& gq, float k,
                                    float& sw, f3& sum) {
  if (px_id(cq) != px_id(p.c) || !finite3(cq)) return;  // a miss, outside the image, another BVH record, or not finite
  const float dot = p.g.x * gq.x + p.g.y * gq.y + p.g.z * gq.z;  // not weight_n: inlined here it inverts a branch of the pass kernels
  float wn = dot > 0.0f ? dot : 0.0f;
  for (int i = 0; i < dp.nsq; ++i) wn = wn * wn;
  const float wz = weight_z(p.g, gq, dp.sigma_d);
  float wc = 1.0f;
  if (pfin) {
    const float dx = p.c.x - cq.x, dy = p.c.y - cq.y, dz = p.c.z - cq.z;
    const float xc = (dx * dx + dy * dy + dz * dz) / (dp.sigma_c * dp.sigma_c);
    wc = 1.0f / ((1.0f + xc) * (1.0f + xc));
  }
  const float w = ((k * wn) * wz) * wc;
  if (!(w > 0.0f)) return;
  sw += w;
  sum.x += w * cq.x;
  sum.y += w * cq.y;
  sum.z += w * cq.z;
}

__device__ __forceinline__ float tap_h(int d) { return d == 0 ? 0.375f : ((d == 1 || d == -1) ? 0.25f : 0.0625f); }

__device__ __forceinline__ f3 resolve(const Px& p, float sw, f3 sum) {
  return sw > 0.0f ? mk(sum.x / sw, sum.y / sw, sum.z / sw) : mk(p.c.x, p.c.y, p.c.z);
}

template <bool FIRST, class P = DParams>
__device__ __forceinline__ void store_px(const P& dp, int i, const Px& p, f3 c) {
  if constexpr (FIRST) dp.guide[i] = p.g;
  if (dp.dst) dp.dst[i] = make_float4(c.x, c.y, c.z, p.c.w);
  if constexpr (kAlbedo<P>) {
    if (!dp.dst && px_id(p.c) != kMissId) c = c * albedo_of(dp, i);  // the last pass: radiance again
  }
  if (dp.out32) dp.out32[i] = make_float4(c.x, c.y, c.z, 1.0f);
  if (dp.out8) dp.out8[i] = pack_srgb8(c);
}

template <bool FIRST, class P = DParams>
__global__ __launch_bounds__(kBlock) void denoise_tiled_kernel(P dp) {
  const int s = dp.step, halo = 2 * s;
  const int sw_px = kTileW + 2 * halo, sh_px = kTileH + 2 * halo, n = sw_px * sh_px;
  float4* lc = g_smem;      // colour | id of the staged pixels, row-major
  float4* lg = g_smem + n;  // normal | t
  const int x0 = (int)blockIdx.x * kTileW - halo, y0 = (int)blockIdx.y * kTileH - halo;
  for (int i = (int)threadIdx.x; i < n; i += kBlock) {
    const int sy = i / sw_px, sx = i - sy * sw_px;
    const int gx = x0 + sx, gy = y0 + sy;
    Px q;
    q.c = make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(kMissId));
    q.g = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (gx >= 0 && gx < dp.W && gy >= 0 && gy < dp.H) q = load_px<FIRST, P>(dp, gy * dp.W + gx);
    lc[i] = q.c;
    lg[i] = q.g;
  }
  __syncthreads();
  const int tx = (int)threadIdx.x & (kTileW - 1), ty = (int)threadIdx.x / kTileW;
  const int x = (int)blockIdx.x * kTileW + tx, y = (int)blockIdx.y * kTileH + ty;
  if (x >= dp.W || y >= dp.H) return;
  const int ci = (ty + halo) * sw_px + tx + halo;
  Px p;
  p.c = ld16(lc + ci);
  p.g = ld16(lg + ci);
  float sw = 0.0f;
  f3 sum = mk(0.0f, 0.0f, 0.0f);
  if (px_id(p.c) != kMissId) {
    const bool pfin = finite3(p.c);
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy) {
#pragma unroll
      for (int dx = -2; dx <= 2; ++dx) {
        const int qi = ci + dy * s * sw_px + dx * s;
        tap(dp, p, pfin, ld16(lc + qi), ld16(lg + qi), tap_h(dx) * tap_h(dy), sw, sum);
      }
    }
  }
  store_px<FIRST, P>(dp, y * dp.W + x, p, resolve(p, sw, sum));
}

template <bool FIRST, class P = DParams>
__global__ __launch_bounds__(kBlock) void denoise_direct_kernel(P dp) {
  const int x = (int)blockIdx.x * kDirectW + ((int)threadIdx.x & (kDirectW - 1));
  const int y = (int)blockIdx.y * kDirectH + (int)threadIdx.x / kDirectW;
  if (x >= dp.W || y >= dp.H) return;
  const int pi = y * dp.W + x;
  const Px p = load_px<FIRST, P>(dp, pi);
  float sw = 0.0f;
  f3 sum = mk(0.0f, 0.0f, 0.0f);
  if (px_id(p.c) != kMissId) {
    const bool pfin = finite3(p.c);
    const int s = dp.step;
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy) {
      const int qy = y + dy * s;
#pragma unroll
      for (int dx = -2; dx <= 2; ++dx) {
        const int qx = x + dx * s;
        if (qx < 0 || qx >= dp.W || qy < 0 || qy >= dp.H) continue;
        const Px q = load_px<FIRST, P>(dp, qy * dp.W + qx);
        tap(dp, p, pfin, q.c, q.g, tap_h(dx) * tap_h(dy), sw, sum);
      }
    }
  }
  store_px<FIRST, P>(dp, pi, p, resolve(p, sw, sum));
}

// passes == 0: the mean and the outputs alone (accumulate_kernel's output stage).
__global__ __launch_bounds__(kBlock) void denoise_resolve_kernel(DParams dp) {
  const int i = (int)(blockIdx.x * kBlock + threadIdx.x);
  if (i >= dp.W * dp.H) return;
  const float4 a = dp.src[i];
  const f3 o = mk(a.x, a.y, a.z) / dp.frames;
  Px p;
  p.c = make_float4(o.x, o.y, o.z, 0.0f);
  p.g = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  store_px<false>(dp, i, p, o);
}

// ---- the variance-guided filter (include/srt_variance.h) ----
//
// 1 + passes launches, all of denoise_direct_kernel's shape: a wave covers 64 contiguous pixels of a row, colour | id
// and normal | t are whole dwordx4 loads and the variance is a dword of an array of its own.
//   variance_resolve_kernel  mean, guide pack and var_0: the temporal variance where the history is long enough,
//                            else a 7 x 7 estimate from the neighbours' moments (three 16-B loads a tap, taken only
//                            by the lanes of young pixels)
//   variance_pass_kernel     one a-trous pass: the 3 x 3 blur of the variance (per neighbour the variance and the id,
//                            a dword each), then the 25 taps with one more dword each; one square root and one more
//                            division per pixel
struct VParams {
  const float4* src;      // resolve: the colour sum; pass: colour | id of the previous launch
  const uint4* hits;      // resolve: the srt_hit records, 2 uint4 each
  const float4* moments;  // resolve: (m1, m2, v, N)
  float4* guide;          // normal | t: written by the resolve, read by the passes
  float4* dst;            // colour | id for the next launch (nullptr in the last pass)
  float4* out32;          // last pass: (colour, 1) or nullptr
  uint32_t* out8;         // last pass: sRGB8 or nullptr
  const float* vsrc;      // pass: var_i
  float* vdst;            // var_{i+1} for the next launch, var_0 from the resolve (nullptr in the last pass)
  float* outv;            // last pass: var_passes or nullptr
  int W, H, step;
  int nsq;
  float frames;           // resolve: float(frames)
  float sigma_d, sigma_l;
  float min_history;      // resolve: float(min_history)
};

__global__ __launch_bounds__(kBlock) void variance_resolve_kernel(VParams vp) {
  const int x = (int)blockIdx.x * kDirectW + ((int)threadIdx.x & (kDirectW - 1));
  const int y = (int)blockIdx.y * kDirectH + (int)threadIdx.x / kDirectW;
  if (x >= vp.W || y >= vp.H) return;
  const int pi = y * vp.W + x;
  const float4 a = ld16(vp.src + pi);
  const uint4 h0 = ld16(vp.hits + 2 * (size_t)pi), h1 = ld16(vp.hits + 2 * (size_t)pi + 1);
  const float4 m = ld16(vp.moments + pi);
  const f3 o = mk(a.x, a.y, a.z) / vp.frames;
  const uint32_t id = hit_id(h0, h1);
  const float4 gp = hit_guide(h0, h1);
  float var = 0.0f;
  if (id != kMissId) {
    if (m.w >= vp.min_history) {
      var = m.z;
    } else {
      float s1 = 0.0f, s2 = 0.0f, sw = 0.0f;
      for (int dy = -3; dy <= 3; ++dy) {
        const int qy = y + dy;
        for (int dx = -3; dx <= 3; ++dx) {
          const int qx = x + dx;
          if (qx < 0 || qx >= vp.W || qy < 0 || qy >= vp.H) continue;
          const int qi = qy * vp.W + qx;
          const uint4 q0 = ld16(vp.hits + 2 * (size_t)qi), q1 = ld16(vp.hits + 2 * (size_t)qi + 1);
          const float4 mq = ld16(vp.moments + qi);
          if (hit_id(q0, q1) != id || !finite1(mq.x) || !finite1(mq.y)) continue;
          const float4 gq = hit_guide(q0, q1);
          const float w = weight_n(gp, gq, vp.nsq) * weight_z(gp, gq, vp.sigma_d);
          s1 += w * mq.x;
          s2 += w * mq.y;
          sw += w;
        }
      }
      if (sw > 0.0f) {
        const float ea = s1 / sw, eb = s2 / sw;
        const float d = eb - ea * ea;
        var = (d > 0.0f ? d : 0.0f) * (vp.min_history / m.w);
      }
    }
  }
  vp.guide[pi] = gp;
  vp.dst[pi] = make_float4(o.x, o.y, o.z, __uint_as_float(id));
  vp.vdst[pi] = var;
}

__global__ __launch_bounds__(kBlock) void variance_pass_kernel(VParams vp) {
  const int x = (int)blockIdx.x * kDirectW + ((int)threadIdx.x & (kDirectW - 1));
  const int y = (int)blockIdx.y * kDirectH + (int)threadIdx.x / kDirectW;
  if (x >= vp.W || y >= vp.H) return;
  const int pi = y * vp.W + x;
  Px p;
  p.c = ld16(vp.src + pi);
  p.g = ld16(vp.guide + pi);
  f3 c = mk(p.c.x, p.c.y, p.c.z);
  float var = 0.0f;
  if (px_id(p.c) != kMissId) {
    var = vp.vsrc[pi];
    // the variance blurred over the 3 x 3 neighbours, whatever the step
    float sg = 0.0f, sk = 0.0f;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy) {
      const int qy = y + dy;
#pragma unroll
      for (int dx = -1; dx <= 1; ++dx) {
        const int qx = x + dx;
        if (qx < 0 || qx >= vp.W || qy < 0 || qy >= vp.H) continue;
        const int qi = qy * vp.W + qx;
        const uint32_t qid = __float_as_uint(reinterpret_cast<const float*>(vp.src + qi)[3]);
        const float vq = vp.vsrc[qi];
        if (qid != px_id(p.c) || !finite1(vq)) continue;
        const float kg = (dx == 0 ? 0.5f : 0.25f) * (dy == 0 ? 0.5f : 0.25f);
        sg += kg * vq;
        sk += kg;
      }
    }
    const float g = sk > 0.0f ? sg / sk : 0.0f;
    const float sl = vp.sigma_l * __builtin_sqrtf(g) + 1e-4f;
    const float Lp = lum(p.c.x, p.c.y, p.c.z);
    const bool lfin = finite1(Lp);
    float sw = 0.0f, sv = 0.0f;
    f3 sum = mk(0.0f, 0.0f, 0.0f);
    const int s = vp.step;
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy) {
      const int qy = y + dy * s;
#pragma unroll
      for (int dx = -2; dx <= 2; ++dx) {
        const int qx = x + dx * s;
        if (qx < 0 || qx >= vp.W || qy < 0 || qy >= vp.H) continue;
        const int qi = qy * vp.W + qx;
        const float4 cq = ld16(vp.src + qi), gq = ld16(vp.guide + qi);
        const float vq = vp.vsrc[qi];
        if (px_id(cq) != px_id(p.c) || !finite3(cq)) continue;
        float wl = 1.0f;
        if (lfin) {
          const float xl = __builtin_fabsf(Lp - lum(cq.x, cq.y, cq.z)) / sl;
          wl = 1.0f / ((1.0f + xl) * (1.0f + xl));
        }
        const float w = (((tap_h(dx) * tap_h(dy)) * weight_n(p.g, gq, vp.nsq)) * weight_z(p.g, gq, vp.sigma_d)) * wl;
        if (!(w > 0.0f)) continue;
        sw += w;
        sum.x += w * cq.x;
        sum.y += w * cq.y;
        sum.z += w * cq.z;
        if (finite1(vq)) sv += (w * w) * vq;
      }
    }
    if (sw > 0.0f) {
      c = mk(sum.x / sw, sum.y / sw, sum.z / sw);
      var = sv / (sw * sw);
    }
  }
  if (vp.dst) vp.dst[pi] = make_float4(c.x, c.y, c.z, p.c.w);
  if (vp.vdst) vp.vdst[pi] = var;
  if (vp.out32) vp.out32[pi] = make_float4(c.x, c.y, c.z, 1.0f);
  if (vp.out8) {  // not pack_srgb8: inlined here it swaps two operands of the kernel's v_or3_b32
    const uint32_t r = to_unorm8(linearToSrgb(c.x)), g = to_unorm8(linearToSrgb(c.y)), b = to_unorm8(linearToSrgb(c.z));
    vp.out8[pi] = r | (g << 8) | (b << 16) | (255u << 24);
  }
  if (vp.outv) vp.outv[pi] = var;
}

struct RayParams {
  float4* rays;  // 2 float4 per srt_ray: origin | pad0, direction | intersection_distance
  int W, H;
  float o[3], p00[3], du[3], dv[3];
};

__global__ __launch_bounds__(kBlock) void primary_rays_kernel(RayParams rp) {
  const int p = (int)(blockIdx.x * kBlock + threadIdx.x);
  if (p >= rp.W * rp.H) return;
  const int j = p / rp.W, i = p - j * rp.W;
  const float fi = (float)i, fj = (float)j;
  const float dx = pixel_dir(rp.p00[0], rp.du[0], rp.dv[0], rp.o[0], fi, fj);
  const float dy = pixel_dir(rp.p00[1], rp.du[1], rp.dv[1], rp.o[1], fi, fj);
  const float dz = pixel_dir(rp.p00[2], rp.du[2], rp.dv[2], rp.o[2], fi, fj);
  rp.rays[2 * (size_t)p] = make_float4(rp.o[0], rp.o[1], rp.o[2], 0.0f);
  rp.rays[2 * (size_t)p + 1] = make_float4(dx, dy, dz, 1e30f);
}

}  // namespace denoise
}  // namespace srt
