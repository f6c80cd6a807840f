// rebuild.hip -- the device rebuild of include/srt_rebuild.h: the rebuild data of a query object, the launches of
// rebuild.hpp's kernels around hipcub's radix sort, the one readback, the new schedule and stack plan, the
// refit that fills the boxes, and the hit remap.  A translation unit of its own beside query.hip and refit.hip.
#include <hip/hip_runtime.h>
#include <hipcub/device/device_radix_sort.hpp>

#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "../../include/srt_rebuild.h"
#include "query_object.hpp"
#include "rebuild.hpp"
#include "rebuild_host.hpp"
#include "stage.hpp"

namespace srt {
namespace rebuild {

namespace {

constexpr int kKeyBits = 30;

uint32_t Blocks(uint32_t n) { return (n + kBlock - 1) / kBlock; }

hipError_t Sort(State& st, uint32_t n, hipStream_t stream, void* temp, size_t& temp_bytes) {
  return hipcub::DeviceRadixSort::SortPairs(temp, temp_bytes, (const uint32_t*)st.d_keys_in.get(), st.d_keys.get(),
                                            (const uint32_t*)st.d_vals_in.get(), st.d_order.get(), n, 0, kKeyBits, stream);
}

}  // namespace

int Enable(srt_query* q) {
  STAGE_HIP_OK(hipSetDevice(q->device));
  std::unique_ptr<State> st(new State());
  const uint32_t n = q->n_tris, n_pairs = n - 1;
  const size_t pairs = 4 * sizeof(float4) * (size_t)(n_pairs ? n_pairs : 1u);
  const size_t sched = sizeof(uint32_t) * ((size_t)n_pairs + kHeightBins + 1);
  const size_t per_tri = sizeof(uint32_t) * (size_t)n;
  const size_t zeroed = sizeof(uint32_t) * (2 * (size_t)kHeightBins + n_pairs);
  const size_t box = sizeof(float) * 8 * (1 + (size_t)kBoxBlocks);
  STAGE_HIP_OK(st->d_pairs.Alloc(pairs));
  STAGE_HIP_OK(st->d_triples.Alloc(sizeof(uint4) * (size_t)n));
  STAGE_HIP_OK(st->d_schedule.Alloc(sched));
  STAGE_HIP_OK(st->d_keys_in.Alloc(per_tri));
  STAGE_HIP_OK(st->d_vals_in.Alloc(per_tri));
  STAGE_HIP_OK(st->d_keys.Alloc(per_tri));
  STAGE_HIP_OK(st->d_order.Alloc(per_tri));
  STAGE_HIP_OK(st->d_parent.Alloc(sizeof(uint32_t) * (2 * (size_t)n)));
  STAGE_HIP_OK(st->d_height.Alloc(sizeof(uint32_t) * (size_t)(n_pairs ? n_pairs : 1u)));
  STAGE_HIP_OK(st->d_zeroed.Alloc(zeroed));
  STAGE_HIP_OK(st->d_box.Alloc(box));
  size_t temp = 0;
  STAGE_HIP_OK(Sort(*st, n, q->stream, nullptr, temp));  // the size only
  st->temp_bytes = temp ? temp : 16;
  STAGE_HIP_OK(st->d_temp.Alloc(st->temp_bytes));
  // one triangle: the order is the identity for good (its rebuild is a refit)
  STAGE_HIP_OK(hipMemsetAsync(st->d_order, 0, per_tri, q->stream));
  STAGE_HIP_OK(hipStreamSynchronize(q->stream));
  st->bytes = pairs + sizeof(uint4) * (size_t)n + sched + 4 * per_tri + sizeof(uint32_t) * (2 * (size_t)n) +
              sizeof(uint32_t) * (size_t)(n_pairs ? n_pairs : 1u) + zeroed + box + st->temp_bytes;
  q->rebuild = std::move(st);
  return SRT_OK;
}

int Rebuild(srt_query* q, const srt_vertex* verts_dev) {
  STAGE_HIP_OK(hipSetDevice(q->device));
  State& st = *q->rebuild;
  const uint32_t n = q->n_tris;
  if (n == 1) {  // a leaf root: nothing to sort, the refit is the rebuild
    if (int rc = refit::Enqueue(q, verts_dev)) return rc;
    st.launches = (int)q->schedule.launches;
    st.depth = 0;
    ++st.count;
    return SRT_OK;
  }
  const uint32_t n_pairs = n - 1;
  const bool first_time = st.count == 0;
  if (first_time) {
    // the LBVH's arrays take the object's place; the state keeps the creation-order triples for every later
    // sort, and the replaced tree's pairs and schedule until the synchronisation below
    std::swap(st.d_pairs, q->d_pairs);
    std::swap(st.d_triples, q->d_triples);
    std::swap(st.d_schedule, q->d_schedule);
    const size_t pb = 4 * sizeof(float4) * (size_t)n_pairs, tb = sizeof(uint4) * (size_t)n;
    q->scene_bytes = q->scene_bytes - q->pairs_bytes + pb;
    q->pairs_bytes = pb;
    q->n_pairs = n_pairs;
    q->refit_bytes = tb + sizeof(uint32_t) * ((size_t)n_pairs + kHeightBins + 1);
  }
  BParams bp;
  std::memset(&bp, 0, sizeof bp);
  bp.pairs = q->d_pairs;
  bp.roots = q->d_roots;
  bp.triples0 = st.d_triples;
  bp.triples = q->d_triples;
  bp.verts = reinterpret_cast<const float4*>(verts_dev);
  bp.box = st.d_box;
  bp.box_partial = st.d_box + 8;
  bp.keys_in = st.d_keys_in;
  bp.vals_in = st.d_vals_in;
  bp.keys = st.d_keys;
  bp.order = st.d_order;
  bp.parent = st.d_parent;
  bp.counts = st.d_zeroed;
  bp.cursor = st.d_zeroed + kHeightBins;
  bp.arrive = st.d_zeroed + 2 * kHeightBins;
  bp.height = st.d_height;
  bp.schedule = q->d_schedule;
  bp.n_verts = q->n_verts;
  bp.n_tris = n;
  bp.box_blocks = Blocks(n) < kBoxBlocks ? Blocks(n) : kBoxBlocks;
  hipStream_t s = q->stream;
  int launches = 0;
#define REBUILD_LAUNCH(kernel, blocks)                                            \
  do {                                                                            \
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(kBlock), 0, s, bp);             \
    STAGE_HIP_OK(hipGetLastError());                                              \
    ++launches;                                                                   \
  } while (0)
  STAGE_HIP_OK(hipMemsetAsync(st.d_zeroed, 0, sizeof(uint32_t) * (2 * (size_t)kHeightBins + n_pairs), s));
  REBUILD_LAUNCH(box_partial_kernel, bp.box_blocks);
  REBUILD_LAUNCH(box_final_kernel, 1);
  REBUILD_LAUNCH(keys_kernel, Blocks(n));
  size_t temp = st.temp_bytes;
  STAGE_HIP_OK(Sort(st, n, s, st.d_temp, temp));
  ++launches;  // (the sort's own launches are hipcub's business: counted as one)
  REBUILD_LAUNCH(karras_kernel, Blocks(n_pairs));
  REBUILD_LAUNCH(permute_kernel, Blocks(n));
  REBUILD_LAUNCH(climb_kernel, Blocks(n));
  REBUILD_LAUNCH(schedule_kernel, Blocks(n_pairs));
#undef REBUILD_LAUNCH
  // the one synchronisation: the pair counts per height
  STAGE_HIP_OK(hipMemcpyAsync(st.summary, st.d_zeroed, sizeof(uint32_t) * kHeightBins, hipMemcpyDeviceToHost, s));
  STAGE_HIP_OK(hipStreamSynchronize(s));
  if (first_time) {  // nothing enqueued reads the replaced tree any more
    st.d_pairs.Free();
    st.d_schedule.Free();
  }
  refit::Schedule sched;
  if (!ScheduleFromCounts(st.summary, kHeightBins, n_pairs, &sched)) {
    srt::SetError("srt_query_rebuild: the device hierarchy is not a tree over every triangle (non-finite vertices?)");
    return SRT_ERR_STATE;
  }
  st.summary[kHeightBins] = sched.heights;
  st.summary[kHeightBins + 1] = n_pairs;
  st.tail_first.assign(sched.first.begin() + sched.tail_begin, sched.first.end());
  STAGE_HIP_OK(hipMemcpyAsync(q->d_schedule + n_pairs, st.tail_first.data(), sizeof(uint32_t) * st.tail_first.size(),
                              hipMemcpyHostToDevice, s));
  q->schedule = std::move(sched);
  // the stack plan of the new tree: one-triangle leaves, depth == heights
  query::Layout shape;
  shape.n_pairs = n_pairs;
  shape.max_leaf = 1;
  shape.depth = (int)q->schedule.heights;
  const query::StackPlan plan = query::PlanStack(shape, n);
  const query::StackPlan old = q->plan;
  q->plan = plan;
  if (plan.in_hbm != old.in_hbm || plan.packed != old.packed || plan.lds_bytes != old.lds_bytes)
    if (int rc = query::PlanGrid(q)) return rc;
  if (plan.hbm_block_bytes != old.hbm_block_bytes) {  // the next query allocates the area it needs
    q->d_stack.Free();
    q->stack_blocks = 0;
  }
  if (int rc = refit::Enqueue(q, verts_dev)) return rc;
  st.launches = launches + (int)q->schedule.launches;
  st.depth = shape.depth;
  ++st.count;
  return SRT_OK;
}

int EnqueueRemap(srt_query* q, srt_hit* hits_dev, uint32_t n) {
  static_assert(sizeof(srt_hit) == 8 * sizeof(uint32_t), "remap_kernel strides by 8 dwords");
  hipLaunchKernelGGL(remap_kernel, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, q->stream,
                     reinterpret_cast<uint32_t*>(hits_dev), (const uint32_t*)q->rebuild->d_order.get(), n, q->n_tris);
  STAGE_HIP_OK(hipGetLastError());
  return SRT_OK;
}

}  // namespace rebuild
}  // namespace srt

extern "C" {

int srt_rebuild_abi_version(void) { return SRT_REBUILD_ABI_VERSION; }

int srt_bvh_build_lbvh(const srt_triangle* tris, uint32_t n_tris, const srt_vertex* verts, uint32_t n_verts,
                       srt_bvh_node* nodes_out, srt_triangle* tris_out, uint32_t* order_out) {
  std::string err;
  const int rc = srt::rebuild::BuildLBVH(tris, n_tris, verts, n_verts, nodes_out, tris_out, order_out, &err);
  if (rc) srt::SetError(err);
  return rc;
}

int srt_query_enable_rebuild(srt_query* q) {
  std::string err;
  if (int rc = srt::rebuild::CheckEnable(q != nullptr, q && q->refit, q ? q->n_bvhs : 0, q ? q->first_index0 : 0,
                                         q ? q->n_tris : 0, &err)) {
    srt::SetError(err);
    return rc;
  }
  if (q->rebuild) return SRT_OK;
  return srt::rebuild::Enable(q);
}

int srt_query_rebuild(srt_query* q, const srt_vertex* verts_dev, uint32_t n_verts) {
  std::string err;
  if (int rc = srt::rebuild::CheckRebuild(q != nullptr, q && q->refit, q && q->rebuild, verts_dev, n_verts,
                                          q ? q->n_verts : 0, &err)) {
    srt::SetError(err);
    return rc;
  }
  return srt::rebuild::Rebuild(q, verts_dev);
}

int srt_query_tri_order(srt_query* q, uint32_t* order_host, uint32_t n) {
  if (!q || !order_host) return SRT_ERR_INVALID;
  // (an object without SRT_QUERY_REFIT does not keep its triangle count: any n is the identity there)
  if (q->refit && n != q->n_tris) {
    srt::SetError("srt_query_tri_order: n differs from the object's triangle count");
    return SRT_ERR_INVALID;
  }
  STAGE_HIP_OK(hipSetDevice(q->device));
  STAGE_HIP_OK(hipStreamSynchronize(q->stream));
  if (!q->rebuild || q->rebuild->count == 0 || q->n_tris == 1) {
    for (uint32_t i = 0; i < n; ++i) order_host[i] = i;
    return SRT_OK;
  }
  STAGE_HIP_OK(hipMemcpy(order_host, q->rebuild->d_order, sizeof(uint32_t) * (size_t)n, hipMemcpyDeviceToHost));
  return SRT_OK;
}

}  // extern "C"
