// upsample.hpp -- the kernel of the guided upsampler (include/srt_upsample.h; DESIGN.md section 5, "Guided
// upsampling").
//
// One launch.  A 256-lane block owns a 32 x 8 tile of full-resolution pixels, one lane each.  The taps of a tile
// (bilinear stage, rescue ring, nearest pixel) lie in a footprint of at most (32 / f + 4) x (8 / f + 4) low pixels,
// each read by up to 16 f^2 lanes.  A low pixel is two float4 as in denoise.hpp: colour | id (the mean; id: the BVH
// record of its hit as bits, all ones for a miss) and normal | t.
//   upsample_kernel<true>   the footprint staged once in LDS (the accumulation sum and the 32-B srt_hit record per
//                           low pixel: three dwordx4 loads, the mean's division once, two ds_write_b128); taps are
//                           ds_read_b128 pairs
//   upsample_kernel<false>  every tap three global dwordx4 loads and the mean's division, as denoise_direct_kernel's
//                           first pass
// A low pixel outside the image is staged (or fetched) with a NaN colour: the contract's finite test then skips it,
// for a hit and for a miss pixel alike.  The arithmetic is the contract's (fp32, source order, no contraction,
// correctly rounded division).  The 16-B loads, the hit unpacking, the normal and depth weights and the sRGB8 encode
// are image_device.hpp's, shared with denoise.hpp.
#pragma once

#include "image_device.hpp"
#include "upsample_host.hpp"

namespace srt {
namespace upsample {
using namespace dev;
using namespace image;

struct UParams {
  const float4* src;       // the low accumulation image (sum | 1)
  const uint4* low_hits;   // the low guide: srt_hit records, 2 uint4 each
  const uint4* full_hits;  // the full guide
  float4* out32;           // (result, 1) or nullptr
  uint32_t* out8;          // sRGB8 or nullptr
  int w, h;                // low size
  int W, H;                // full size
  int f;                   // factor
  int foot_w, foot_h;      // footprint of a block (staged variant)
  int nsq;                 // normal_squarings
  float frames;            // float(frames)
  float sigma_d;
};

struct Px {
  float4 c;  // colour | id
  float4 g;  // normal | t
};

__device__ __forceinline__ uint32_t px_id(const float4& c) { return __float_as_uint(c.w); }
__device__ __forceinline__ bool finite3(const float4& c) { return finite1(c.x) && finite1(c.y) && finite1(c.z); }

// The low pixel (i, j): its mean and packed guide, or a NaN colour outside the image.
__device__ __forceinline__ Px load_low(const UParams& up, int i, int j) {
  Px r;
  if (i < 0 || i >= up.w || j < 0 || j >= up.h) {
    const float nan = __uint_as_float(0x7FC00000u);
    r.c = make_float4(nan, nan, nan, __uint_as_float(kMissId));
    r.g = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    return r;
  }
  const size_t q = (size_t)j * (size_t)up.w + (size_t)i;
  const float4 a = ld16(up.src + q);
  const uint4 h0 = ld16(up.low_hits + 2 * q), h1 = ld16(up.low_hits + 2 * q + 1);
  const f3 o = mk(a.x, a.y, a.z) / up.frames;
  r.c = make_float4(o.x, o.y, o.z, __uint_as_float(hit_id(h0, h1)));
  r.g = hit_guide(h0, h1);
  return r;
}

// n = 2X + 1 - f, i0 = floor(n / 2f), r = n - 2f * i0, a1 = float(r) / float(2f), a0 = 1 - a1.
__device__ __forceinline__ void axis_terms(int X, int f, int& i0, float& a0, float& a1) {
  const int n = 2 * X + 1 - f;
  i0 = FloorDiv(n, 2 * f);
  const int r = n - 2 * f * i0;
  a1 = (float)r / (float)(2 * f);
  a0 = 1.0f - a1;
}

// One tap of the pixel with id `pid` and guide `gp`; `k` is the bilinear weight, or 1 in the rescue ring
// ((1 * wn) * wz is wn * wz bit for bit).
__device__ __forceinline__ void tap(const UParams& up, uint32_t pid, const float4& gp, const Px& q, float k, float& sw,
                                    f3& sum) {
  if (px_id(q.c) != pid || !finite3(q.c)) return;  // another id, outside the image, or not finite
  float w = k;
  if (pid != kMissId) w = (k * weight_n(gp, q.g, up.nsq)) * weight_z(gp, q.g, up.sigma_d);
  if (!(w > 0.0f)) return;
  sum.x = sum.x + w * q.c.x;
  sum.y = sum.y + w * q.c.y;
  sum.z = sum.z + w * q.c.z;
  sw = sw + w;
}

template <bool STAGED>
__global__ __launch_bounds__(kBlock) void upsample_kernel(UParams up) {
  const int f = up.f;
  const int X0 = (int)blockIdx.x * kTileW, Y0 = (int)blockIdx.y * kTileH;
  const int lx = FootOrigin(X0, f), ly = FootOrigin(Y0, f);
  float4* lc = g_smem;  // colour | id of the staged low pixels, row-major
  float4* lg = g_smem;  // normal | t
  if constexpr (STAGED) {
    const int n = up.foot_w * up.foot_h;
    lg = g_smem + n;
    for (int i = (int)threadIdx.x; i < n; i += kBlock) {
      const int sy = i / up.foot_w, sx = i - sy * up.foot_w;
      const Px q = load_low(up, lx + sx, ly + sy);
      lc[i] = q.c;
      lg[i] = q.g;
    }
    __syncthreads();
  }
  const int X = X0 + ((int)threadIdx.x & (kTileW - 1)), Y = Y0 + (int)threadIdx.x / kTileW;
  if (X >= up.W || Y >= up.H) return;
  const size_t P = (size_t)Y * (size_t)up.W + (size_t)X;
  const uint4 h0 = ld16(up.full_hits + 2 * P), h1 = ld16(up.full_hits + 2 * P + 1);
  const uint32_t pid = hit_id(h0, h1);
  const float4 gp = hit_guide(h0, h1);
  auto fetch = [&](int i, int j) -> Px {
    if constexpr (STAGED) {
      const int s = (j - ly) * up.foot_w + (i - lx);
      Px q;
      q.c = ld16(lc + s);
      q.g = ld16(lg + s);
      return q;
    } else {
      return load_low(up, i, j);
    }
  };
  int i0, j0;
  float a[2], b[2];
  axis_terms(X, f, i0, a[0], a[1]);
  axis_terms(Y, f, j0, b[0], b[1]);
  float sw = 0.0f;
  f3 sum = mk(0.0f, 0.0f, 0.0f);
#pragma unroll
  for (int dy = 0; dy < 2; ++dy) {
#pragma unroll
    for (int dx = 0; dx < 2; ++dx) tap(up, pid, gp, fetch(i0 + dx, j0 + dy), a[dx] * b[dy], sw, sum);
  }
  if (!(sw > 0.0f)) {  // the rescue ring: the 4 x 4 low pixels around the bilinear four, those included
    sw = 0.0f;
    sum = mk(0.0f, 0.0f, 0.0f);
#pragma unroll 1
    for (int dy = -1; dy <= 2; ++dy) {
#pragma unroll 1
      for (int dx = -1; dx <= 2; ++dx) tap(up, pid, gp, fetch(i0 + dx, j0 + dy), 1.0f, sw, sum);
    }
  }
  f3 c;
  if (sw > 0.0f) {
    c = mk(sum.x / sw, sum.y / sw, sum.z / sw);
  } else {  // the nearest low pixel as it is
    const Px q = fetch(X / f, Y / f);
    c = mk(q.c.x, q.c.y, q.c.z);
  }
  if (up.out32) up.out32[P] = make_float4(c.x, c.y, c.z, 1.0f);
  if (up.out8) up.out8[P] = pack_srgb8(c);
}

}  // namespace upsample
}  // namespace srt
