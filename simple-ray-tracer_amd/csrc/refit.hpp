// refit.hpp -- the device BVH refit (include/srt_refit.h) over query_host.hpp's layout: the argument of
// refit_kernels.hpp's kernels and the policy that instantiates them.  One schedule entry is a sibling pair, both of
// whose records are refit; an internal record's child pair is the pair it names, a leaf's fold starts at the
// triple it names; a triangle's record lies at its index, and after its heights the tail's block refits the roots.
#pragma once

#include "refit_kernels.hpp"

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

struct PairLayout {
  using Params = RParams;
  using Entry = uint32_t;
  static __device__ __forceinline__ const float4* children(const RParams& rp, uint32_t ref) { return rp.pairs + 4 * (size_t)ref; }
  static __device__ __forceinline__ uint32_t leaf_first(uint32_t ref, uint32_t) { return ref; }
  static __device__ __forceinline__ void refit_entry(const RParams& rp, uint32_t p) {
    float4* rec = rp.pairs + 4 * (size_t)p;
    refit_record<PairLayout>(rp, rec, p);
    refit_record<PairLayout>(rp, rec + 2, p);
  }
  static __device__ __forceinline__ float4* tri_record(const RParams& rp, const uint4&, uint32_t t) { return rp.tris + 3 * (size_t)t; }
  static __device__ __forceinline__ float4 tri_tail(const float4*, const uint4& idx, uint32_t t, float e2z) {
    return make_float4(e2z, __uint_as_float(idx.w), __uint_as_float(t), 0.0f);  // | material, index, 0
  }
  static __device__ __forceinline__ void finish(const RParams& rp) {
    for (uint32_t r = threadIdx.x; r < rp.n_roots; r += kBlock) refit_record<PairLayout>(rp, rp.roots + 2 * (size_t)r, r);
  }
};

}  // namespace refit
}  // namespace srt
