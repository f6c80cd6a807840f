// refit.hip -- the BVH refit of include/srt_refit.h: the host refit's C entry point, the refit data of a query
// object created with SRT_QUERY_REFIT, the launches of refit_kernels.hpp's kernels, and the layout readback.  A
// translation unit of its own beside query.hip, which creates the object (query_object.hpp).
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>
#include <vector>

#include "../../include/srt_refit.h"
#include "query_object.hpp"
#include "refit.hpp"
#include "refit_host.hpp"
#include "stage.hpp"

namespace srt {
namespace refit {

int Attach(srt_query* q, const query::Layout& lay, const srt_triangle* tris, uint32_t n_tris, uint32_t n_verts) {
  static_assert(sizeof(srt_triangle) == sizeof(uint4), "the index triples are uploaded as they are");
  Schedule s = BuildSchedule(lay);
  // the device schedule: the pair indices by height, then the offsets of the tail's levels
  std::vector<uint32_t> sched(s.order);
  sched.insert(sched.end(), s.first.begin() + s.tail_begin, s.first.end());
  const size_t tb = (size_t)n_tris * sizeof(uint4), sb = sched.size() * sizeof(uint32_t);
  STAGE_HIP_OK(q->d_triples.Alloc(tb));
  STAGE_HIP_OK(q->d_schedule.Alloc(sb));
  STAGE_HIP_OK(hipMemcpyAsync(q->d_triples, tris, tb, hipMemcpyHostToDevice, q->stream));
  STAGE_HIP_OK(hipMemcpyAsync(q->d_schedule, sched.data(), sb, hipMemcpyHostToDevice, q->stream));
  STAGE_HIP_OK(hipStreamSynchronize(q->stream));  // the host arrays go out of scope
  q->n_pairs = lay.n_pairs;
  q->n_tris = n_tris;
  q->n_verts = n_verts;
  q->refit_bytes = tb + sb;
  s.order = std::vector<uint32_t>();
  q->schedule = std::move(s);
  q->refit = true;
  return SRT_OK;
}

int Enqueue(srt_query* q, const srt_vertex* verts_dev) {
  STAGE_HIP_OK(hipSetDevice(q->device));
  RParams rp;
  std::memset(&rp, 0, sizeof rp);
  rp.pairs = q->d_pairs;
  rp.roots = q->d_roots;
  rp.tris = q->d_tris;
  rp.triples = q->d_triples;
  rp.order = q->d_schedule;
  rp.tail_first = q->d_schedule + q->n_pairs;
  rp.verts = reinterpret_cast<const float4*>(verts_dev);
  rp.n_verts = q->n_verts;
  rp.n_tris = q->n_tris;
  rp.n_roots = q->n_bvhs + 1;
  return Enqueue<PairLayout>(q->stream, rp, q->schedule);
}

}  // namespace refit
}  // namespace srt

extern "C" {

int srt_refit_abi_version(void) { return SRT_REFIT_ABI_VERSION; }

int srt_bvh_refit(const srt_bvh_record* bvhs, uint32_t n_bvhs, srt_bvh_node* nodes, uint32_t n_nodes,
                  const srt_triangle* tris, uint32_t n_tris, const srt_vertex* verts, uint32_t n_verts) {
  std::string err;
  const int rc = srt::refit::RefitNodes(bvhs, n_bvhs, nodes, n_nodes, tris, n_tris, verts, n_verts, &err);
  if (rc) srt::SetError(err);
  return rc;
}

int srt_query_refit(srt_query* q, const srt_vertex* verts_dev, uint32_t n_verts) {
  if (!q) return SRT_ERR_INVALID;
  if (!q->refit) {
    srt::SetError("srt_query_refit: the object was created without SRT_QUERY_REFIT");
    return SRT_ERR_INVALID;
  }
  if (!verts_dev || !srt::stage::Aligned(verts_dev, 16)) {
    srt::SetError("srt_query_refit: verts_dev must be a 16-byte aligned device pointer");
    return SRT_ERR_INVALID;
  }
  if (n_verts != q->n_verts) {
    srt::SetError("srt_query_refit: n_verts differs from the count at creation");
    return SRT_ERR_INVALID;
  }
  if (int rc = srt::refit::Enqueue(q, verts_dev)) return rc;
  ++q->refit_count;
  return SRT_OK;
}

int srt_query_copy_layout(srt_query* q, void* pairs, void* roots, void* tris) {
  if (!q) return SRT_ERR_INVALID;
  STAGE_HIP_OK(hipSetDevice(q->device));
  STAGE_HIP_OK(hipStreamSynchronize(q->stream));
  if (pairs) STAGE_HIP_OK(hipMemcpy(pairs, q->d_pairs, q->pairs_bytes, hipMemcpyDeviceToHost));
  if (roots) STAGE_HIP_OK(hipMemcpy(roots, q->d_roots, q->roots_bytes, hipMemcpyDeviceToHost));
  if (tris) STAGE_HIP_OK(hipMemcpy(tris, q->d_tris, q->tris_bytes, hipMemcpyDeviceToHost));
  return SRT_OK;
}

}  // extern "C"
