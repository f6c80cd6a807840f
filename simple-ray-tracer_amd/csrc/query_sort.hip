// query_sort.hip -- the sorted ray queries of include/srt_query_sort.h: the scratch of the ordering, the launches in front
// of the traversal (query_sort.hpp's two kernels around hipcub's radix sort), the readback of the last permutation, and
// the C entry of the host mirror.  The traversal itself is query.hip's (EnqueueTrace with the sorted order).  A
// translation unit of its own beside query.hip, so the sort's templates are compiled once, here.
#include <hip/hip_runtime.h>
#include <hipcub/device/device_radix_sort.hpp>

#include <algorithm>
#include <string>

#include "../../include/srt_query_sort.h"
#include "query_object.hpp"
#include "query_sort.hpp"
#include "ray_order_host.hpp"
#include "stage.hpp"

namespace {

using srt::rayorder::kBlock;
using srt::rayorder::kWords;
using srt::rayorder::SParams;
using srt::rayorder::State;

// Stable, as every radix sort is; exactly the key's bits.
hipError_t Sort(const State& st, uint32_t n, hipStream_t stream, void* temp, size_t& temp_bytes) {
  return hipcub::DeviceRadixSort::SortPairs(temp, temp_bytes, (const uint32_t*)st.keys_in(), st.keys(),
                                            (const uint32_t*)st.order_in(), st.order(), (int)n, 0, srt::rayorder::kKeyBits,
                                            stream);
}

// The scratch for n rays: 16 B a ray, the sort's temporary storage and the bounds words.  Allocates only when n exceeds
// what the object holds (hipFree waits for the launches that still read the old arrays).
int Reserve(srt_query* q, uint32_t n) {
  if (!q->sort) q->sort.reset(new State());
  State& st = *q->sort;
  if (!st.d_words) STAGE_HIP_OK(st.d_words.Alloc(kWords * sizeof(uint32_t)));
  if (n > st.capacity) {
    st.capacity = 0;
    STAGE_HIP_OK(st.d_pairs.Alloc(4 * sizeof(uint32_t) * (size_t)n));
    st.capacity = n;
  }
  size_t need = 0;
  STAGE_HIP_OK(Sort(st, n, q->stream, nullptr, need));  // (the size only: nothing is launched)
  if (need > st.temp_bytes) {
    st.temp_bytes = 0;
    STAGE_HIP_OK(st.d_temp.Alloc(need));
    st.temp_bytes = need;
  }
  st.bytes = 4 * sizeof(uint32_t) * (size_t)st.capacity + st.temp_bytes + kWords * sizeof(uint32_t);
  return SRT_OK;
}

int Sorted(srt_query* q, bool any, const srt_ray* rays, uint32_t n, void* out) {
  // what the unsorted call refuses, refused the same way and before anything is allocated or enqueued
  if (!q || (n && (!rays || !out))) return SRT_ERR_INVALID;
  if (n == 0) return SRT_OK;
  if (!srt::stage::Aligned(rays, 16) || (!any && !srt::stage::Aligned(out, 16))) {
    srt::SetError("srt_query: rays and hits must be 16-byte aligned");
    return SRT_ERR_INVALID;
  }
  std::string err;
  if (int rc = srt::rayorder::CheckSorted(n, &err)) {
    srt::SetError(err);
    return rc;
  }
  STAGE_HIP_OK(hipSetDevice(q->device));
  if (int rc = Reserve(q, n)) return rc;
  State& st = *q->sort;
  hipStream_t s = q->stream;
  SParams sp;
  sp.rays = reinterpret_cast<const float4*>(rays);
  sp.words = st.d_words;
  sp.keys_in = st.keys_in();
  sp.order_in = st.order_in();
  sp.n = n;
  const uint32_t blocks = (n + kBlock - 1) / kBlock;
  STAGE_HIP_OK(hipMemsetAsync(st.d_words, 0, kWords * sizeof(uint32_t), s));
  hipLaunchKernelGGL(srt::rayorder::ray_bounds_kernel, dim3(std::min(blocks, srt::rayorder::kBoundsBlocks)), dim3(kBlock), 0,
                     s, sp);
  STAGE_HIP_OK(hipGetLastError());
  hipLaunchKernelGGL(srt::rayorder::ray_keys_kernel, dim3(blocks), dim3(kBlock), 0, s, sp);
  STAGE_HIP_OK(hipGetLastError());
  size_t temp_bytes = st.temp_bytes;
  STAGE_HIP_OK(Sort(st, n, s, st.d_temp, temp_bytes));
  int launches = 3;  // (the sort's own launches are hipcub's business: counted as one)
  if (int rc = srt::query::EnqueueTrace(q, any, rays, n, out, st.order())) return rc;
  ++launches;
  // a rebuilt object holds its triangle records in the LBVH's order (include/srt_rebuild.h)
  if (!any && q->rebuild && q->rebuild->count > 0) {
    if (int rc = srt::rebuild::EnqueueRemap(q, static_cast<srt_hit*>(out), n)) return rc;
    ++launches;
  }
  st.last_n = n;
  st.launches = launches;
  ++st.count;
  return SRT_OK;
}

}  // namespace

extern "C" {

int srt_query_sort_abi_version(void) { return SRT_QUERY_SORT_ABI_VERSION; }

int srt_query_closest_sorted(srt_query* q, const srt_ray* rays_dev, uint32_t n, srt_hit* hits_dev) {
  return Sorted(q, false, rays_dev, n, hits_dev);
}

int srt_query_occluded_sorted(srt_query* q, const srt_ray* rays_dev, uint32_t n, uint8_t* occluded_dev) {
  return Sorted(q, true, rays_dev, n, occluded_dev);
}

int srt_ray_order(const srt_ray* rays, uint32_t n, uint32_t* order, uint32_t* keys, float* bounds) {
  std::string err;
  const int rc = srt::rayorder::RayOrder(rays, n, order, keys, bounds, &err);
  if (rc) srt::SetError(err);
  return rc;
}

int srt_query_copy_ray_order(srt_query* q, uint32_t* order, uint32_t* keys, uint32_t n) {
  if (!q) return SRT_ERR_INVALID;
  if (!q->sort || q->sort->count == 0 || n != q->sort->last_n) {
    srt::SetError("srt_query_copy_ray_order: no sorted call has run, or n differs from the last one's");
    return SRT_ERR_STATE;
  }
  const State& st = *q->sort;
  STAGE_HIP_OK(hipSetDevice(q->device));
  STAGE_HIP_OK(hipStreamSynchronize(q->stream));
  if (order) STAGE_HIP_OK(hipMemcpy(order, st.order(), sizeof(uint32_t) * (size_t)n, hipMemcpyDeviceToHost));
  if (keys) STAGE_HIP_OK(hipMemcpy(keys, st.keys(), sizeof(uint32_t) * (size_t)n, hipMemcpyDeviceToHost));
  return SRT_OK;
}

}  // extern "C"
