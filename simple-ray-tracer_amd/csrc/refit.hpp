// refit.hpp -- the kernels of the device BVH refit (include/srt_refit.h) over query_host.hpp's layout.
//
// refit_tris_kernel: one lane per triangle, three 16-B gathers through the index triple, three 16-B stores.
// refit_level_kernel: one lane per sibling pair of one height; both slots by the header's single rule -- a leaf
// slot folds its triangles' vertices, gathered through the index triples (never v0 + e1, a different float), an
// internal slot folds the two boxes of its child pair, which an earlier launch (or an earlier level of the same
// block) wrote.  refit_tail_kernel: one 256-lane block walks the last levels, none wider than the block, with a
// block barrier between them, then the roots.  No block waits on another: the order between levels is the
// stream's or the barrier's.  Selects and two subtractions only, so every dword equals the host's.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "refit_fold.hpp"

namespace srt {
namespace refit {

struct RParams {
  float4* pairs;              // 4 float4 per sibling pair
  float4* roots;              // 2 float4 per root record
  float4* tris;               // 3 float4 per triangle
  const uint4* triples;       // v0, v1, v2, material per triangle
  const uint32_t* order;      // pair indices by height
  const uint32_t* tail_first; // tail_levels + 1 offsets into `order`
  const float4* verts;        // 2 float4 per srt_vertex; the first holds the position
  uint32_t n_verts, n_tris, n_roots, tail_levels;
};

// (Box, opaque, fold and the position gather: refit_fold.hpp, shared with the path tracer's scene refit)
__device__ __forceinline__ float4 load_vert(const RParams& rp, uint32_t i) { return load_pos(rp.verts, rp.n_verts, i); }

// The box of one slot: (ref, cnt) are its .w fields, which stay.
__device__ __forceinline__ Box slot_box(const RParams& rp, uint32_t ref, uint32_t cnt) {
  Box b;
  if (cnt > 0u) {
    uint4 t = rp.triples[ref];
    float4 a = load_vert(rp, t.x);
    b.lo[0] = b.hi[0] = a.x;
    b.lo[1] = b.hi[1] = a.y;
    b.lo[2] = b.hi[2] = a.z;
    for (uint32_t k = 0;;) {  // a per-lane loop: the builder's leaves hold 1 or 2 triangles
      fold(b, a);
      fold(b, load_vert(rp, t.y));
      fold(b, load_vert(rp, t.z));
      if (++k == cnt) break;
      t = rp.triples[(size_t)ref + k];
      a = load_vert(rp, t.x);
    }
  } else {
    const float4* p = rp.pairs + 4 * (size_t)ref;
    const float4 l0 = p[0], h0 = p[1], l1 = p[2], h1 = p[3];
    b.lo[0] = l1.x < l0.x ? l1.x : l0.x;
    b.lo[1] = l1.y < l0.y ? l1.y : l0.y;
    b.lo[2] = l1.z < l0.z ? l1.z : l0.z;
    b.hi[0] = h1.x > h0.x ? h1.x : h0.x;
    b.hi[1] = h1.y > h0.y ? h1.y : h0.y;
    b.hi[2] = h1.z > h0.z ? h1.z : h0.z;
  }
  return b;
}

// One record (min | ref) (max | cnt) at rec[0], rec[1].
__device__ __forceinline__ void refit_record(const RParams& rp, float4* rec) {
  const float ref = opaque(rec[0].w), cnt = opaque(rec[1].w);
  const Box b = slot_box(rp, __float_as_uint(ref), __float_as_uint(cnt));
  rec[0] = make_float4(b.lo[0], b.lo[1], b.lo[2], ref);
  rec[1] = make_float4(b.hi[0], b.hi[1], b.hi[2], cnt);
}

__device__ __forceinline__ void refit_pair(const RParams& rp, uint32_t p) {
  float4* rec = rp.pairs + 4 * (size_t)p;
  refit_record(rp, rec);
  refit_record(rp, rec + 2);
}

__global__ __launch_bounds__(256) void refit_tris_kernel(RParams rp) {
  const uint32_t t = blockIdx.x * 256u + threadIdx.x;
  if (t >= rp.n_tris) return;
  const uint4 idx = rp.triples[t];
  const float4 a = load_vert(rp, idx.x), b = load_vert(rp, idx.y), c = load_vert(rp, idx.z);
  const float e1x = b.x - a.x, e1y = b.y - a.y, e1z = b.z - a.z;
  const float e2x = c.x - a.x, e2y = c.y - a.y, e2z = c.z - a.z;
  float4* o = rp.tris + 3 * (size_t)t;
  o[0] = make_float4(a.x, a.y, a.z, e1x);
  o[1] = make_float4(e1y, e1z, e2x, e2y);
  o[2] = make_float4(e2z, __uint_as_float(idx.w), __uint_as_float(t), 0.0f);
}

__global__ __launch_bounds__(256) void refit_level_kernel(RParams rp, uint32_t first, uint32_t count) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i < count) refit_pair(rp, rp.order[(size_t)first + i]);
}

__global__ __launch_bounds__(256) void refit_tail_kernel(RParams rp) {
  for (uint32_t l = 0; l < rp.tail_levels; ++l) {  // (uniform: every lane reaches every barrier)
    const uint32_t first = rp.tail_first[l], count = rp.tail_first[l + 1] - first;
    if (threadIdx.x < count) refit_pair(rp, rp.order[(size_t)first + threadIdx.x]);
    __syncthreads();  // the level's stores are visible to the block before the next level reads them
  }
  for (uint32_t r = threadIdx.x; r < rp.n_roots; r += 256u) refit_record(rp, rp.roots + 2 * (size_t)r);
}

}  // namespace refit
}  // namespace srt
