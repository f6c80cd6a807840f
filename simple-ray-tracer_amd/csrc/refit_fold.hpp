// refit_fold.hpp -- the device helpers both refits share (refit.hpp over the query layout, scene_refit.hpp over the
// path tracer's): the fold of include/srt_refit.h, the position gather and the register fence that keeps an
// access at 16 B.
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

}  // namespace refit
}  // namespace srt
