// refit_kernels.hpp -- the three kernels of a device refit and their launches, once, for the query refit (refit.hpp:
// sibling pairs) and the path tracer's scene refit (scene_refit.hpp: node slots).  A layout policy L says what differs:
//   L::Params, L::Entry            the kernels' argument (with triples, verts, n_verts, n_tris, order, tail_first,
//                                  tail_levels) and what its `order` holds
//   L::refit_entry(p, e)           refits what one entry stands for, through refit_record<L> and store_box
//   L::children(p, ref)            the four float4 of the child pair an internal record's `ref` names
//   L::leaf_first(ref, e)          the index triple a leaf's fold starts at
//   L::tri_record(p, idx, t)       where triangle t's three float4 go (idx: its index triple)
//   L::tri_tail(o, idx, t, e2z)    the record's third float4: e2.z and the layout's own three dwords
//   L::finish(p)                   what the tail's block does after its heights
//
// tris_kernel: one lane per triangle.  level_kernel: one lane per entry of one height.  tail_kernel: one kBlock-lane
// block walks the last heights, none wider than the block, with a block barrier between them.  No block waits on
// another: the order between heights is the stream's or the barrier's.  Launch-bound (profiles/refit.json): no LDS, a
// few registers; every store, gather and box load is one 16-B access, kept whole by opaque() -- but a record's own two
// .w fields, read as single dwords, and the schedule entries.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "refit_fold.hpp"
#include "refit_levels.hpp"
#include "stage.hpp"

namespace srt {
namespace refit {

// Refits the record (min | ref) (max | cnt) at rec[0], rec[1] by the header's single rule -- a leaf (cnt > 0) folds its
// triangles' vertices, an internal record the two boxes of its child pair -- and returns the box.  The .w fields stay.
template <class L>
__device__ __forceinline__ Box refit_record(const typename L::Params& p, float4* rec, typename L::Entry e) {
  const float ref = opaque(rec[0].w), cnt = opaque(rec[1].w);
  const Box b = __float_as_uint(cnt) > 0u
                    ? leaf_box(p.triples, p.verts, p.n_verts, L::leaf_first(__float_as_uint(ref), e), __float_as_uint(cnt))
                    : pair_box(L::children(p, __float_as_uint(ref)));
  store_box(rec, b, ref, cnt);
  return b;
}

template <class L>
__global__ __launch_bounds__(kBlock) void tris_kernel(typename L::Params p) {
  const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
  if (t >= p.n_tris) return;
  const uint4 idx = p.triples[t];
  const float4 a = load_pos(p.verts, p.n_verts, idx.x), b = load_pos(p.verts, p.n_verts, idx.y),
               c = load_pos(p.verts, p.n_verts, idx.z);
  const float e1x = b.x - a.x, e1y = b.y - a.y, e1z = b.z - a.z;
  const float e2x = c.x - a.x, e2y = c.y - a.y, e2z = c.z - a.z;
  float4* o = L::tri_record(p, idx, t);
  const float4 tail = L::tri_tail(o, idx, t, e2z);
  o[0] = make_float4(a.x, a.y, a.z, e1x);
  o[1] = make_float4(e1y, e1z, e2x, e2y);
  o[2] = tail;
}

template <class L>
__global__ __launch_bounds__(kBlock) void level_kernel(typename L::Params p, uint32_t first, uint32_t count) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i < count) L::refit_entry(p, p.order[(size_t)first + i]);
}

template <class L>
__global__ __launch_bounds__(kBlock) void tail_kernel(typename L::Params p) {
  for (uint32_t l = 0; l < p.tail_levels; ++l) {  // (uniform: every lane reaches every barrier)
    const uint32_t first = p.tail_first[l], count = p.tail_first[l + 1] - first;
    if (threadIdx.x < count) L::refit_entry(p, p.order[(size_t)first + threadIdx.x]);
    __syncthreads();  // the height's stores are visible to the block before the next height reads them
  }
  L::finish(p);
}

// One refit on `stream`: the triangle records, a launch per height below the tail, the tail (p.tail_levels is set here).
template <class L>
int Enqueue(hipStream_t stream, typename L::Params p, const Levels& lv) {
  p.tail_levels = lv.heights - lv.tail_begin;
  if (p.n_tris > 0) {
    hipLaunchKernelGGL(tris_kernel<L>, dim3((p.n_tris + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, p);
    STAGE_HIP_OK(hipGetLastError());
  }
  for (uint32_t h = 0; h < lv.tail_begin; ++h) {
    const uint32_t first = lv.first[h], count = lv.first[h + 1] - first;
    hipLaunchKernelGGL(level_kernel<L>, dim3((count + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, p, first, count);
    STAGE_HIP_OK(hipGetLastError());
  }
  hipLaunchKernelGGL(tail_kernel<L>, dim3(1), dim3(kBlock), 0, stream, p);
  STAGE_HIP_OK(hipGetLastError());
  return SRT_OK;
}

}  // namespace refit
}  // namespace srt
