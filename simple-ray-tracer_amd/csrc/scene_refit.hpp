// scene_refit.hpp -- the kernels of the path tracer's scene refit (include/srt_scene_refit.h) over the device
// layout of scene_image.hpp: node records (min | ref) (max | cnt) at float4 2 * slot + 2 of the node array, an
// internal record's children at slots (ref | ref_or) and the next, triangle records v0 e1 e2 | material, input
// index, 0 at float4 3 * slot of the triangle array.
//
// tris_kernel: one lane per input triangle, three 16-B gathers through the index triple, three 16-B stores at
// the triangle's slot (the third record's material, input index and zero are read and stored back).
// level_kernel: one lane per node of one height -- a leaf folds its triangles' vertices, gathered through the
// index triples in input order (never v0 + e1, a different float), an internal node folds the boxes of its child
// pair, which an earlier launch (or an earlier height of the same block) wrote -- and stores the box into the
// node array and, where there is one, its treelet copy, each with the record's own .w fields.  tail_kernel: one
// 256-lane block walks the last heights, none wider than the block, with a block barrier between them.  No
// block waits on another: the order between heights is the stream's or the barrier's.  Selects and two
// subtractions only, so every dword equals the host's.  Launch-bound like refit.hpp's (profiles/refit.json): no
// LDS, a few registers; every store, every position gather and every box or record load is one 16-B access, kept
// whole by opaque() -- the exceptions are a node's own two .w fields, read as single dwords, and the 8-B schedule
// entries.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "refit_fold.hpp"

namespace srt {
namespace scene_refit {

using refit::Box;
using refit::fold;
using refit::load_pos;
using refit::opaque;

struct SParams {
  float4* nodes;              // the node array (behind its 32-B pad: record s at nodes[2 s + 2])
  float4* nodes_t;            // its treelet copy, or null
  float4* tris;               // 3 float4 per triangle slot
  const uint4* triples;       // per input triangle: v0, v1, v2, slot
  const uint2* order;         // (node slot, a leaf's first input triangle) by height
  const uint32_t* tail_first; // tail_levels + 1 offsets into `order`
  const float4* verts;        // 2 float4 per srt_vertex; the first holds the position
  uint32_t n_verts, n_tris, ref_or, tail_levels;
};

// opaque() for an index record's dword: a leaf's fold does not use the slot in .w, and the load stays 16 B.
__device__ __forceinline__ uint4 load_triple(const SParams& sp, size_t i) {
  uint4 t = sp.triples[i];
  asm volatile("" : "+v"(t.w));
  return t;
}

__device__ __forceinline__ void store_box(float4* rec, const Box& b) {
  const float ref = opaque(rec[0].w), cnt = opaque(rec[1].w);
  rec[0] = make_float4(b.lo[0], b.lo[1], b.lo[2], ref);
  rec[1] = make_float4(b.hi[0], b.hi[1], b.hi[2], cnt);
}

__device__ __forceinline__ void refit_node(const SParams& sp, uint2 e) {
  float4* rec = sp.nodes + 2 * (size_t)e.x + 2;
  const uint32_t ref = __float_as_uint(rec[0].w), cnt = __float_as_uint(rec[1].w);
  Box b;
  if (cnt > 0u) {
    uint4 t = load_triple(sp, e.y);
    float4 a = load_pos(sp.verts, sp.n_verts, t.x);
    b.lo[0] = b.hi[0] = a.x;
    b.lo[1] = b.hi[1] = a.y;
    b.lo[2] = b.hi[2] = a.z;
    for (uint32_t k = 0;;) {  // a per-lane loop: the builder's leaves hold 1 or 2 triangles
      fold(b, a);
      fold(b, load_pos(sp.verts, sp.n_verts, t.y));
      fold(b, load_pos(sp.verts, sp.n_verts, t.z));
      if (++k == cnt) break;
      t = load_triple(sp, (size_t)e.y + k);
      a = load_pos(sp.verts, sp.n_verts, t.x);
    }
  } else {
    const float4* p = sp.nodes + 2 * (size_t)(ref | sp.ref_or) + 2;
    float4 l0 = p[0], h0 = p[1], l1 = p[2], h1 = p[3];
    l0.w = opaque(l0.w);  // (the children's .w are not used: fenced, so that the four loads stay 16 B)
    h0.w = opaque(h0.w);
    l1.w = opaque(l1.w);
    h1.w = opaque(h1.w);
    b.lo[0] = l1.x < l0.x ? l1.x : l0.x;
    b.lo[1] = l1.y < l0.y ? l1.y : l0.y;
    b.lo[2] = l1.z < l0.z ? l1.z : l0.z;
    b.hi[0] = h1.x > h0.x ? h1.x : h0.x;
    b.hi[1] = h1.y > h0.y ? h1.y : h0.y;
    b.hi[2] = h1.z > h0.z ? h1.z : h0.z;
  }
  store_box(rec, b);
  if (sp.nodes_t) store_box(sp.nodes_t + 2 * (size_t)e.x + 2, b);  // (uniform: one array or both for a launch)
}

__global__ __launch_bounds__(256) void tris_kernel(SParams sp) {
  const uint32_t t = blockIdx.x * 256u + threadIdx.x;
  if (t >= sp.n_tris) return;
  const uint4 idx = sp.triples[t];
  const float4 a = load_pos(sp.verts, sp.n_verts, idx.x), b = load_pos(sp.verts, sp.n_verts, idx.y),
               c = load_pos(sp.verts, sp.n_verts, idx.z);
  const float e1x = b.x - a.x, e1y = b.y - a.y, e1z = b.z - a.z;
  const float e2x = c.x - a.x, e2y = c.y - a.y, e2z = c.z - a.z;
  float4* o = sp.tris + 3 * (size_t)idx.w;
  float4 keep = o[2];  // material, input index, 0
  keep.x = opaque(keep.x);  // (replaced below: fenced, so that the load stays 16 B)
  o[0] = make_float4(a.x, a.y, a.z, e1x);
  o[1] = make_float4(e1y, e1z, e2x, e2y);
  o[2] = make_float4(e2z, opaque(keep.y), opaque(keep.z), opaque(keep.w));
}

__global__ __launch_bounds__(256) void level_kernel(SParams sp, uint32_t first, uint32_t count) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i < count) refit_node(sp, sp.order[(size_t)first + i]);
}

__global__ __launch_bounds__(256) void tail_kernel(SParams sp) {
  for (uint32_t l = 0; l < sp.tail_levels; ++l) {  // (uniform: every lane reaches every barrier)
    const uint32_t first = sp.tail_first[l], count = sp.tail_first[l + 1] - first;
    if (threadIdx.x < count) refit_node(sp, sp.order[(size_t)first + threadIdx.x]);
    __syncthreads();  // the height's stores are visible to the block before the next height reads them
  }
}

}  // namespace scene_refit
}  // namespace srt
