// image_device.hpp -- device helpers the image stages share (denoise.hpp, temporal.hpp, surface.hpp), each stated
// once: the variance filter reads the moments temporal.hpp wrote, so the luminance, the hit unpacking and the
// weights must be the same expressions bit for bit.  pathtrace.hip and the headers it includes never include this
// file (it is no part of the device code srt_code_hash identifies); device_common.hpp is only read, for the sRGB8
// encode.  The arithmetic is the contract's (fp32, source order, no contraction, correctly rounded division).
#pragma once

#include "device_common.hpp"

namespace srt {
namespace image {

constexpr uint32_t kMissId = 0xFFFFFFFFu;  // the id of a miss, or of a pixel outside the image

__device__ __forceinline__ bool finite1(float v) { return (__float_as_uint(v) & 0x7F800000u) != 0x7F800000u; }

// A whole 16-B word in one instruction (dwordx4 / ds_read_b128): the empty asm makes all four components
// live, or the compiler splits the load at the component that is tested first.
typedef float v4f __attribute__((ext_vector_type(4)));
typedef uint32_t v4u __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float4 ld16(const float4* p) {
  v4f v = *reinterpret_cast<const v4f*>(p);
  asm("" : "+v"(v));
  return make_float4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ uint4 ld16(const uint4* p) {
  v4u v = *reinterpret_cast<const v4u*>(p);
  asm("" : "+v"(v));
  return make_uint4(v.x, v.y, v.z, v.w);
}

// Rec. 709 luminance.
__device__ __forceinline__ float lum(float x, float y, float z) { return (0.2126f * x + 0.7152f * y) + 0.0722f * z; }

// An srt_hit as its two 16-B words (triangle t n.x n.y | n.z material bvh pad): the id is the hit's BVH record,
// all ones for a miss; the guide is normal | t.
__device__ __forceinline__ uint32_t hit_id(const uint4& h0, const uint4& h1) { return h0.x == kMissId ? kMissId : h1.z; }
__device__ __forceinline__ float4 hit_guide(const uint4& h0, const uint4& h1) {
  return make_float4(__uint_as_float(h0.z), __uint_as_float(h0.w), __uint_as_float(h1.x), __uint_as_float(h0.y));
}

// The edge-stopping weights of two guides (normal | t): the clamped cosine squared `nsq` times, and the relative
// depth difference over sigma_d.
__device__ __forceinline__ float weight_n(const float4& gp, const float4& gq, int nsq) {
  const float dot = gp.x * gq.x + gp.y * gq.y + gp.z * gq.z;
  float wn = dot > 0.0f ? dot : 0.0f;
  for (int i = 0; i < nsq; ++i) wn = wn * wn;
  return wn;
}
__device__ __forceinline__ float weight_z(const float4& gp, const float4& gq, float sigma_d) {
  const float xz = __builtin_fabsf(gp.w - gq.w) / (sigma_d * (gp.w + gq.w));
  return 1.0f / ((1.0f + xz) * (1.0f + xz));
}

// A linear colour as sRGB8 (device_common.hpp's linearToSrgb / to_unorm8, as accumulate_kernel uses them), alpha 255.
__device__ __forceinline__ uint32_t pack_srgb8(f3 c) {
  const uint32_t r = to_unorm8(linearToSrgb(c.x)), g = to_unorm8(linearToSrgb(c.y)), b = to_unorm8(linearToSrgb(c.z));
  return r | (g << 8) | (b << 16) | (255u << 24);
}

// One component of the direction of pixel (i, j)'s centre ray in denoise_host.hpp's PrimaryBasis (unnormalised).
__device__ __forceinline__ float pixel_dir(float p00, float du, float dv, float o, float fi, float fj) {
  return ((p00 + fi * du) + fj * dv) - o;
}

}  // namespace image
}  // namespace srt
