// refit_fold.hpp -- the device rules every refit shares (refit_kernels.hpp builds the query refit's and the path
// tracer's kernels from them; rebuild.hpp folds its scene box with them): the fold of include/srt_refit.h, the
// position gather, the box of a leaf and of a child pair, the store that keeps a record's own .w fields, and the
// register fence that keeps an access at 16 B.  Selects only, so every dword equals the host's.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace srt {
namespace refit {

struct Box {
  float lo[3], hi[3];
};

// Keeps a register's value out of the optimiser's sight, so that an access stays the 16 B it is written as: a
// position's unused pad would narrow its gather to 12 B, and a record's unchanged .w its store.
__device__ __forceinline__ float opaque(float v) {
  asm volatile("" : "+v"(v));
  return v;
}

// The position of vertex i: `verts` holds 2 float4 per srt_vertex, the first the position; past n_verts, zeros.
__device__ __forceinline__ float4 load_pos(const float4* verts, uint32_t n_verts, uint32_t i) {
  float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  if (i < n_verts) {
    v = verts[2 * (size_t)i];
    v.w = opaque(v.w);
  }
  return v;
}

__device__ __forceinline__ void fold(Box& b, const float4& v) {
  b.lo[0] = v.x < b.lo[0] ? v.x : b.lo[0];
  b.lo[1] = v.y < b.lo[1] ? v.y : b.lo[1];
  b.lo[2] = v.z < b.lo[2] ? v.z : b.lo[2];
  b.hi[0] = v.x > b.hi[0] ? v.x : b.hi[0];
  b.hi[1] = v.y > b.hi[1] ? v.y : b.hi[1];
  b.hi[2] = v.z > b.hi[2] ? v.z : b.hi[2];
}

// An index triple for a fold, which does not use its .w (a material or a slot): fenced, and the load stays 16 B.
__device__ __forceinline__ uint4 load_triple(const uint4* triples, size_t i) {
  uint4 t = triples[i];
  asm volatile("" : "+v"(t.w));
  return t;
}

// The leaf rule: the box of the vertices of triples first .. first+cnt-1 (cnt >= 1), gathered through the index
// triples (never v0 + e1, a different float) and seeded from the first triple's v0.
__device__ __forceinline__ Box leaf_box(const uint4* triples, const float4* verts, uint32_t n_verts, uint32_t first,
                                        uint32_t cnt) {
  Box b;
  uint4 t = load_triple(triples, first);
  float4 a = load_pos(verts, n_verts, t.x);
  b.lo[0] = b.hi[0] = a.x;
  b.lo[1] = b.hi[1] = a.y;
  b.lo[2] = b.hi[2] = a.z;
  for (uint32_t k = 0;;) {  // a per-lane loop: a host-built leaf holds a few triangles, a rebuilt one up to 255
    fold(b, a);
    fold(b, load_pos(verts, n_verts, t.y));
    fold(b, load_pos(verts, n_verts, t.z));
    if (++k == cnt) break;
    t = load_triple(triples, (size_t)first + k);
    a = load_pos(verts, n_verts, t.x);
  }
  return b;
}

// The box of a child pair: p[0 .. 3] are its two records, (min | ref) (max | cnt) each, which an earlier launch (or an
// earlier height of the same block) wrote.  (The children's .w are not used: fenced, so that the four loads stay 16 B.)
__device__ __forceinline__ Box pair_box(const float4* p) {
  float4 l0 = p[0], h0 = p[1], l1 = p[2], h1 = p[3];
  l0.w = opaque(l0.w), h0.w = opaque(h0.w), l1.w = opaque(l1.w), h1.w = opaque(h1.w);
  Box b;
  b.lo[0] = l1.x < l0.x ? l1.x : l0.x;
  b.lo[1] = l1.y < l0.y ? l1.y : l0.y;
  b.lo[2] = l1.z < l0.z ? l1.z : l0.z;
  b.hi[0] = h1.x > h0.x ? h1.x : h0.x;
  b.hi[1] = h1.y > h0.y ? h1.y : h0.y;
  b.hi[2] = h1.z > h0.z ? h1.z : h0.z;
  return b;
}

// One record (min | ref) (max | cnt) at rec[0], rec[1]: the box goes in, the record's own .w fields stay.
__device__ __forceinline__ void store_box(float4* rec, const Box& b, float ref, float cnt) {
  rec[0] = make_float4(b.lo[0], b.lo[1], b.lo[2], ref);
  rec[1] = make_float4(b.hi[0], b.hi[1], b.hi[2], cnt);
}
__device__ __forceinline__ void store_box(float4* rec, const Box& b) { store_box(rec, b, opaque(rec[0].w), opaque(rec[1].w)); }

}  // namespace refit
}  // namespace srt
