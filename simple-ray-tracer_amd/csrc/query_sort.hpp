// query_sort.hpp -- the two kernels in front of a sorted ray query (include/srt_query_sort.h); the rule is
// ray_order_rule.hpp's, the sort between them and the traversal hipcub's and query.hpp's.
//
// ray_bounds_kernel: a grid-stride loop over the rays, one 16-B load each (the origin); every lane folds its rays into six
//   words of its own (rule 1), a wave reduces them by shuffles, the block's four waves through LDS, and lanes 0..5 issue
//   one atomic max each on the launch's six words, zeroed before it.  A maximum of words is exact and commutes, so the
//   result does not depend on the grid or on the order of arrival.
// ray_keys_kernel: one lane per ray, two 16-B loads (origin, direction); the six words are read through wave-uniform
//   addresses; the ray's key (rules 2-4) and its own index as the sort's value.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "ray_order_rule.hpp"

namespace srt {
namespace rayorder {

constexpr uint32_t kBlock = 256;
constexpr uint32_t kBoundsBlocks = 1024;  // most blocks of the bounds kernel: 4 a CU of a 256-CU device

struct SParams {
  const float4* rays;  // 2 float4 per ray
  uint32_t* words;     // kWords, zero at ray_bounds_kernel's launch
  uint32_t* keys_in;   // n
  uint32_t* order_in;  // n
  uint32_t n;
};

__global__ __launch_bounds__(256) void ray_bounds_kernel(SParams sp) {
  __shared__ uint32_t sh[kBlock / 64][kWords];
  uint32_t w[kWords] = {0u, 0u, 0u, 0u, 0u, 0u};
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < sp.n; i += (uint64_t)gridDim.x * kBlock) {
    const float4 o = sp.rays[2 * i];
    Fold(w, o.x, o.y, o.z);
  }
  for (int off = 32; off > 0; off >>= 1) {
    uint32_t o[kWords];
    for (int k = 0; k < kWords; ++k) o[k] = (uint32_t)__shfl_xor((int)w[k], off, 64);
    Merge(w, o);
  }
  if ((threadIdx.x & 63u) == 0u)
    for (int k = 0; k < kWords; ++k) sh[threadIdx.x >> 6][k] = w[k];
  __syncthreads();
  if (threadIdx.x < (uint32_t)kWords) {
    uint32_t m = sh[0][threadIdx.x];
    for (uint32_t v = 1; v < kBlock / 64; ++v) m = sh[v][threadIdx.x] > m ? sh[v][threadIdx.x] : m;
    if (m != 0u) atomicMax(sp.words + threadIdx.x, m);  // (zero: the block saw no finite value on this axis)
  }
}

__global__ __launch_bounds__(256) void ray_keys_kernel(SParams sp) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= sp.n) return;
  uint32_t w[kWords];
  for (int k = 0; k < kWords; ++k) w[k] = sp.words[k];
  const Bounds b = Decode(w);
  const float4 o = sp.rays[2 * (size_t)i], d = sp.rays[2 * (size_t)i + 1];
  sp.keys_in[i] = Key(b, o.x, o.y, o.z, d.x, d.y, d.z);
  sp.order_in[i] = i;
}

}  // namespace rayorder
}  // namespace srt
