// surface.hpp -- surface_shade_kernel: albedo, barycentrics and uv of closest-hit records
// (include/srt_surface.h; DESIGN.md section 5, "Surface attributes and demodulation").
//
// One lane per ray, 256-lane blocks.  A lane moves its srt_hit, its srt_ray and its srt_surface_attr as two
// dwordx4 each; a miss lane stores zeros after the hit record alone.  A hit lane gathers the frame of the hit's
// BVH record (4 x 16 B), its triangle (4 x 16 B: v0, e1, e2, material, the three uvs) and the material (16 B),
// and a sampled material reads four texels, a dword each.  The arithmetic is TriangleToSupportedMat's as
// shading.hpp's mesh_texture_albedo / texture_sample state it (contract A: fp32, source order, no contraction,
// dot with fused multiply-adds, correctly rounded division), restated here over this stage's own parameters;
// pt_math.hpp is only read.
#pragma once

#include "image_device.hpp"
#include "surface_host.hpp"

namespace srt {
namespace surface {
using namespace dev;
using namespace image;

struct SParams {
  const float4* frames;     // 4 float4 (the columns) per BVH record, n_bvhs + 1 records (the last: zeros)
  const float4* tris;       // 4 float4 per triangle
  const float4* mats;       // 1 float4 per material
  const uint32_t* texels;   // r | g << 8 | b << 16 of all textures
  const uint4* tex_info;    // per texture: first texel, width, height, 0
  const float4* rays;       // 2 float4 per srt_ray
  const uint4* hits;        // 2 uint4 per srt_hit
  float4* out;              // 2 float4 per srt_surface_attr
  uint32_t n;
  uint32_t n_bvhs, bvh_count, n_tris, n_tex;
};

// A whole 16-B word in one store, as image_device.hpp's ld16 loads one.
__device__ __forceinline__ void st16(float4* p, float x, float y, float z, float w) {
  v4f v = {x, y, z, w};
  *reinterpret_cast<v4f*>(p) = v;
}

// traversal.hpp's xform over the frame's columns: ((m0 * x + m4 * y) + m8 * z) + m12 * w per row
__device__ __forceinline__ f3 xform4(const float4& c0, const float4& c1, const float4& c2, const float4& c3, f3 v, float w) {
  return mk(((c0.x * v.x + c1.x * v.y) + c2.x * v.z) + c3.x * w,
            ((c0.y * v.x + c1.y * v.y) + c2.y * v.z) + c3.y * w,
            ((c0.z * v.x + c1.z * v.y) + c2.z * v.z) + c3.z * w);
}

// c / 255 correctly rounded (shading.hpp's unorm8: q = c * RN(1/255) and one Markstein correction, equal to the
// IEEE quotient for all 256 values)
__device__ __forceinline__ float texel_unorm8(uint32_t p, int sh) {
  constexpr float kInv255 = 0.003921568859368563f;
  const float c = (float)((p >> sh) & 255u);
  const float q = c * kInv255;
  return __builtin_fmaf(__builtin_fmaf(-255.0f, q, c), kInv255, q);
}

// texture(sampler2D, vec2(s, t)).xyz at level 0, GL_LINEAR, GL_REPEAT (the sampling contract).
// i0 and j0 are held inside the texture whatever s * w rounds to, so no read leaves it.
__device__ __forceinline__ f3 sample_bilinear(const SParams& sp, uint32_t tex, float s, float t) {
  const uint4 info = sp.tex_info[tex];
  const int w = (int)info.y, h = (int)info.z;
  if (!(__builtin_fabsf(s) <= 3.402823466e38f)) s = 0.0f;
  if (!(__builtin_fabsf(t) <= 3.402823466e38f)) t = 0.0f;
  s = s - __builtin_floorf(s);
  t = t - __builtin_floorf(t);
  const float x = s * (float)w - 0.5f, y = t * (float)h - 0.5f;
  const float fx = __builtin_floorf(x), fy = __builtin_floorf(y);
  const float a = x - fx, b = y - fy;
  int i0 = f2i(fx), j0 = f2i(fy);
  i0 = i0 < 0 ? w - 1 : (i0 > w - 1 ? w - 1 : i0);
  j0 = j0 < 0 ? h - 1 : (j0 > h - 1 ? h - 1 : j0);
  int i1 = f2i(fx) < 0 ? 0 : i0 + 1, j1 = f2i(fy) < 0 ? 0 : j0 + 1;
  i1 = i1 >= w ? 0 : i1;
  j1 = j1 >= h ? 0 : j1;
  const float w00 = (1.0f - a) * (1.0f - b), w10 = a * (1.0f - b), w01 = (1.0f - a) * b, w11 = a * b;
  const uint32_t* T = sp.texels + info.x;
  const uint32_t p00 = T[(uint32_t)j0 * (uint32_t)w + (uint32_t)i0], p10 = T[(uint32_t)j0 * (uint32_t)w + (uint32_t)i1];
  const uint32_t p01 = T[(uint32_t)j1 * (uint32_t)w + (uint32_t)i0], p11 = T[(uint32_t)j1 * (uint32_t)w + (uint32_t)i1];
  float c[3];
#pragma unroll
  for (int k = 0; k < 3; ++k)
    c[k] = ((w00 * texel_unorm8(p00, 8 * k) + w10 * texel_unorm8(p10, 8 * k)) + w01 * texel_unorm8(p01, 8 * k)) +
           w11 * texel_unorm8(p11, 8 * k);
  return mk(c[0], c[1], c[2]);
}

__global__ __launch_bounds__(kBlock) void surface_shade_kernel(SParams sp) {
  const uint32_t i = blockIdx.x * (uint32_t)kBlock + threadIdx.x;
  if (i >= sp.n) return;
  const uint4 h0 = ld16(sp.hits + 2 * (size_t)i), h1 = ld16(sp.hits + 2 * (size_t)i + 1);  // triangle t n.x n.y | n.z material bvh pad
  float4* const o = sp.out + 2 * (size_t)i;
  const uint32_t tri = h0.x;
  if (tri >= sp.n_tris) {  // a miss (kMissId), or an index no triangle of the scene has
    st16(o, 0.0f, 0.0f, 0.0f, 0.0f);
    st16(o + 1, 0.0f, 0.0f, 0.0f, 0.0f);
    return;
  }
  const float4 r0 = ld16(sp.rays + 2 * (size_t)i), r1 = ld16(sp.rays + 2 * (size_t)i + 1);
  const uint32_t b = (h1.z < sp.bvh_count && h1.z < sp.n_bvhs) ? h1.z : sp.n_bvhs;  // past the count: the zero record
  const float4* fr = sp.frames + 4 * (size_t)b;
  const float4 c0 = ld16(fr), c1 = ld16(fr + 1), c2 = ld16(fr + 2), c3 = ld16(fr + 3);
  const float4* tp = sp.tris + 4 * (size_t)tri;
  const float4 A = ld16(tp), B = ld16(tp + 1), C = ld16(tp + 2), D = ld16(tp + 3);
  const float4 m = ld16(sp.mats + __float_as_uint(C.y));
  // model_p in the hit BVH's frame (raytrace_compute.glsl:155) and the barycentrics of mesh_texture_albedo
  const f3 to = xform4(c0, c1, c2, c3, mk(r0.x, r0.y, r0.z), 1.0f), td = xform4(c0, c1, c2, c3, mk(r1.x, r1.y, r1.z), 0.0f);
  const f3 mp = (__uint_as_float(h0.y) * td) + to;
  const f3 v0 = mk(A.x, A.y, A.z), v0v1 = mk(A.w, B.x, B.y), v0v2 = mk(B.z, B.w, C.x);
  const f3 v0p = mp - v0;
  const float d00 = dot(v0v1, v0v1), d01 = dot(v0v1, v0v2), d11 = dot(v0v2, v0v2);
  const float d20 = dot(v0p, v0v1), d21 = dot(v0p, v0v2);
  const float denom = 1.0f / (d00 * d11 - d01 * d01);
  const float v = (d11 * d20 - d01 * d21) * denom;
  const float w = (d00 * d21 - d01 * d20) * denom;
  const float u = 1.0f - v - w;
  const float s = (u * C.z + v * D.x) + w * D.z;
  const float t = (u * C.w + v * D.y) + w * D.w;
  f3 alb = mk(m.x, m.y, m.z);
  if (__float_as_uint(m.w) != 0u) {  // sampled: (handle[0], handle[1]); an unknown handle gives zero
    const uint32_t tex = __float_as_uint(m.x);
    alb = mk(0.0f, 0.0f, 0.0f);
    if (__float_as_uint(m.y) == 0u && tex < sp.n_tex) alb = sample_bilinear(sp, tex, s, t);
  }
  st16(o, alb.x, alb.y, alb.z, v);
  st16(o + 1, w, s, t, __uint_as_float(1u));
}

// srt_surface_refit (include/srt_surface_refit.h): one lane per triangle, three 16-B gathers through the index
// triple, and the record's first three words rewritten -- v0, v1 - v0, v2 - v0, the two subtractions
// surface_host.cpp's BuildLayout makes; the material index and uv0 of the third word are carried over, the fourth
// word (uv1 | uv2) is not touched.  `triples` holds n_tris records whose indices srt_surface_create held below n_verts.
__global__ __launch_bounds__(kBlock) void surface_refit_kernel(float4* __restrict__ tris, const uint4* __restrict__ triples,
                                                               const float4* __restrict__ verts, uint32_t n_tris,
                                                               uint32_t n_verts) {
  const uint32_t t = blockIdx.x * (uint32_t)kBlock + threadIdx.x;
  if (t >= n_tris) return;
  const uint4 idx = ld16(triples + t);
  if (idx.x >= n_verts || idx.y >= n_verts || idx.z >= n_verts) return;  // (validated at creation: never taken)
  const float4 a = ld16(verts + 2 * (size_t)idx.x), b = ld16(verts + 2 * (size_t)idx.y), c = ld16(verts + 2 * (size_t)idx.z);
  float4* const o = tris + 4 * (size_t)t;
  const float4 keep = ld16(o + 2);  // e2.z, material, uv0
  st16(o, a.x, a.y, a.z, b.x - a.x);
  st16(o + 1, b.y - a.y, b.z - a.z, c.x - a.x, c.y - a.y);
  st16(o + 2, c.z - a.z, keep.y, keep.z, keep.w);
}

}  // namespace surface
}  // namespace srt
