// scene_refit.hpp -- the path tracer's scene refit (include/srt_scene_refit.h) over the device layout of
// scene_image.hpp: the argument of refit_kernels.hpp's kernels and the policy that instantiates them.  Node records
// (min | ref) (max | cnt) lie at float4 2 * slot + 2 of the node array, an internal record's children at slots
// (ref | ref_or) and the next, triangle records v0 e1 e2 | material, input index, 0 at float4 3 * slot of the
// triangle array.  One schedule entry is a node slot and, for a leaf, its first input triangle: the fold walks the
// index triples in input order, and the box goes into the node array and, where there is one, its treelet copy,
// each with the record's own .w fields.  A triangle's record goes to the slot its index triple names, and its
// material, input index and zero are read and stored back.
#pragma once

#include "refit_kernels.hpp"

namespace srt {
namespace scene_refit {

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

struct SlotLayout {
  using Params = SParams;
  using Entry = uint2;
  static __device__ __forceinline__ const float4* children(const SParams& sp, uint32_t ref) {
    return sp.nodes + 2 * (size_t)(ref | sp.ref_or) + 2;
  }
  static __device__ __forceinline__ uint32_t leaf_first(uint32_t, uint2 e) { return e.y; }
  static __device__ __forceinline__ void refit_entry(const SParams& sp, uint2 e) {
    const refit::Box b = refit::refit_record<SlotLayout>(sp, sp.nodes + 2 * (size_t)e.x + 2, e);
    if (sp.nodes_t) refit::store_box(sp.nodes_t + 2 * (size_t)e.x + 2, b);  // (uniform: one array or both for a launch)
  }
  static __device__ __forceinline__ float4* tri_record(const SParams& sp, const uint4& idx, uint32_t) { return sp.tris + 3 * (size_t)idx.w; }
  static __device__ __forceinline__ float4 tri_tail(const float4* o, const uint4&, uint32_t, float e2z) {
    float4 keep = o[2];  // material, input index, 0
    keep.x = refit::opaque(keep.x);  // (replaced: fenced, so that the load stays 16 B)
    return make_float4(e2z, refit::opaque(keep.y), refit::opaque(keep.z), refit::opaque(keep.w));
  }
  static __device__ __forceinline__ void finish(const SParams&) {}
};

}  // namespace scene_refit
}  // namespace srt
