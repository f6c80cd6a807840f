// query.hip -- the ray-query service of include/srt_query.h: a device copy of the scene in
// query_host.hpp's layout, and the launches of query_kernel (query.hpp).  A translation unit of its own:
// pathtrace.hip and its headers (the device code srt_code_hash identifies) are only read.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/srt_query.h"
#include "../../include/srt_refit.h"
#include "query.hpp"
#include "query_host.hpp"
#include "query_object.hpp"
#include "ray_order_host.hpp"
#include "stage.hpp"

using srt::stage::Aligned;
using srt::stage::DevPtr;

namespace {

using srt::query::kBlock;
using srt::query::QParams;

// gfx950 hands a block its LDS in units of 1/128 of the CU's 160 KiB; n blocks run together only when
// each asks at most floor(128 / n) units ("occupancy").
int LdsBlocksPerCu(size_t lds) {
  const size_t gran = 160 * 1024 / 128;
  return lds == 0 ? 1 << 30 : (int)(128 / ((lds + gran - 1) / gran));
}

template <bool ANY, bool ORDER>
const void* Instance(bool hbm, bool pack) {
  if (hbm) return pack ? (const void*)srt::query::query_kernel<ANY, true, true, ORDER>
                       : (const void*)srt::query::query_kernel<ANY, true, false, ORDER>;
  return pack ? (const void*)srt::query::query_kernel<ANY, false, true, ORDER>
              : (const void*)srt::query::query_kernel<ANY, false, false, ORDER>;
}

const void* Instance(bool any, bool sorted, bool hbm, bool pack) {
  if (any) return sorted ? Instance<true, true>(hbm, pack) : Instance<true, false>(hbm, pack);
  return sorted ? Instance<false, true>(hbm, pack) : Instance<false, false>(hbm, pack);
}

int Upload(srt_query* q, const srt::query::Layout& lay, const srt_bvh_record* bvhs) {
  std::vector<float> frames(16 * ((size_t)q->n_bvhs + 1), 0.0f);
  for (uint32_t b = 0; b < q->n_bvhs; ++b) std::memcpy(&frames[16 * (size_t)b], bvhs[b].frame, 16 * sizeof(float));
  const size_t pb = lay.pairs.size() * sizeof(float4), rb = lay.roots.size() * sizeof(float4),
               tb = lay.tris.size() * sizeof(float4), fb = frames.size() * sizeof(float);
  STAGE_HIP_OK(q->d_pairs.Alloc(pb));
  STAGE_HIP_OK(q->d_roots.Alloc(rb));
  STAGE_HIP_OK(q->d_tris.Alloc(tb));
  STAGE_HIP_OK(q->d_frames.Alloc(fb));
  STAGE_HIP_OK(q->d_ctr.Alloc(256));
  STAGE_HIP_OK(hipMemcpyAsync(q->d_pairs, lay.pairs.data(), pb, hipMemcpyHostToDevice, q->stream));
  STAGE_HIP_OK(hipMemcpyAsync(q->d_roots, lay.roots.data(), rb, hipMemcpyHostToDevice, q->stream));
  STAGE_HIP_OK(hipMemcpyAsync(q->d_tris, lay.tris.data(), tb, hipMemcpyHostToDevice, q->stream));
  STAGE_HIP_OK(hipMemcpyAsync(q->d_frames, frames.data(), fb, hipMemcpyHostToDevice, q->stream));
  STAGE_HIP_OK(hipStreamSynchronize(q->stream));  // the host arrays go out of scope
  q->scene_bytes = pb + rb + tb + fb;
  q->pairs_bytes = pb;
  q->roots_bytes = rb;
  q->tris_bytes = tb;
  hipDeviceProp_t prop;
  STAGE_HIP_OK(hipGetDeviceProperties(&prop, q->device));
  q->cu_count = prop.multiProcessorCount;
  return srt::query::PlanGrid(q);
}

template <bool ANY>
int Launch(srt_query* q, const srt_ray* rays, uint32_t n, void* out, const uint32_t* order) {
  if (!q || (n && (!rays || !out))) return SRT_ERR_INVALID;
  if (n == 0) return SRT_OK;
  if (!Aligned(rays, 16) || (!ANY && !Aligned(out, 16))) {
    srt::SetError("srt_query: rays and hits must be 16-byte aligned");
    return SRT_ERR_INVALID;
  }
  if (n > 0xFFF00000u) {
    srt::SetError("srt_query: more than 2^32 - 2^20 rays in one call");
    return SRT_ERR_LIMIT;
  }
  STAGE_HIP_OK(hipSetDevice(q->device));
  const int blocks = (int)std::min<uint64_t>((uint64_t)(order ? q->max_blocks_sorted : q->max_blocks)[ANY ? 1 : 0], ((uint64_t)n + kBlock - 1) / kBlock);
  if (q->plan.in_hbm && blocks > q->stack_blocks) {  // grown when n grows (hipFree waits for the device)
    q->d_stack.Free();
    q->stack_blocks = 0;
    STAGE_HIP_OK(q->d_stack.Alloc(q->plan.hbm_block_bytes * (size_t)blocks));
    q->stack_blocks = blocks;
  }
  QParams qp;
  std::memset(&qp, 0, sizeof qp);
  qp.pairs = q->d_pairs;
  qp.roots = q->d_roots;
  qp.tris = q->d_tris;
  qp.frames = q->d_frames;
  qp.rays = reinterpret_cast<const float4*>(rays);
  qp.out = out;
  qp.ctr = q->d_ctr;
  qp.gstack = q->d_stack;
  qp.n = n;
  qp.n_bvhs = q->n_bvhs;
  qp.bvh_count = q->bvh_count;
  // rays per claim: 64, or more (up to 256) while every wave of the grid still claims 8 times or more
  const uint64_t waves = (uint64_t)blocks * (kBlock / 64);
  const uint64_t per = (uint64_t)n / (waves * 64 * 8);
  qp.claim = 64u * (uint32_t)(q->claim_env > 0 ? q->claim_env : std::max<uint64_t>(1, std::min<uint64_t>(4, per)));
  qp.stack_entries = q->plan.entries;
  qp.refill_min = q->refill_min;
  qp.order = order;
  STAGE_HIP_OK(hipMemsetAsync(q->d_ctr, 0, sizeof(uint32_t), q->stream));
  void* args[] = {&qp};
  STAGE_HIP_OK(hipLaunchKernel(Instance(ANY, order != nullptr, q->plan.in_hbm, q->plan.packed), dim3((unsigned)blocks), dim3(kBlock), args,
                          q->plan.lds_bytes, q->stream));
  q->last_blocks = blocks;
  return SRT_OK;
}

}  // namespace

namespace srt {
namespace query {

// persistent grid: the blocks the device holds at once
int PlanGrid(srt_query* q) {
  for (int k = 0; k < 4; ++k) {
    const int any = k & 1, sorted = k >> 1;
    const void* fn = Instance(any != 0, sorted != 0, q->plan.in_hbm, q->plan.packed);
    if (q->plan.lds_bytes > 48 * 1024)
      STAGE_HIP_OK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)q->plan.lds_bytes));
    int per_cu = 0;
    STAGE_HIP_OK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, kBlock, q->plan.lds_bytes));
    per_cu = std::max(1, std::min(per_cu, LdsBlocksPerCu(q->plan.lds_bytes)));
    if (q->plan.in_hbm) per_cu = std::min(per_cu, 4);  // each block holds an HBM stack area
    (sorted ? q->max_blocks_sorted : q->max_blocks)[any] = per_cu * std::max(1, q->cu_count);
  }
  return SRT_OK;
}

int EnqueueTrace(srt_query* q, bool any, const srt_ray* rays, uint32_t n, void* out, const uint32_t* order) {
  return any ? Launch<true>(q, rays, n, out, order) : Launch<false>(q, rays, n, out, order);
}

}  // namespace query
}  // namespace srt

extern "C" {

int srt_query_abi_version(void) { return SRT_QUERY_ABI_VERSION; }

int srt_query_create(int device, void* stream, const srt_bvh_record* bvhs, uint32_t n_bvhs, const srt_bvh_node* nodes,
                     uint32_t n_nodes, const srt_triangle* tris, uint32_t n_tris, const srt_vertex* verts,
                     uint32_t n_verts, srt_query** out) {
  return srt_query_create_ex(device, stream, bvhs, n_bvhs, nodes, n_nodes, tris, n_tris, verts, n_verts, 0, out);
}

int srt_query_create_ex(int device, void* stream, const srt_bvh_record* bvhs, uint32_t n_bvhs, const srt_bvh_node* nodes,
                        uint32_t n_nodes, const srt_triangle* tris, uint32_t n_tris, const srt_vertex* verts,
                        uint32_t n_verts, uint32_t flags, srt_query** out) {
  if (!out) return SRT_ERR_INVALID;
  *out = nullptr;
  if (flags & ~SRT_QUERY_REFIT) {
    srt::SetError("srt_query_create_ex: unknown flags");
    return SRT_ERR_INVALID;
  }
  // host-side validation and re-layout first: a bad scene never reaches the device
  srt::query::Layout lay;
  std::string err;
  if (int rc = srt::query::BuildLayout(bvhs, n_bvhs, nodes, n_nodes, tris, n_tris, verts, n_verts, &lay, &err)) {
    srt::SetError(err);
    return rc;
  }
  if (lay.depth >= (1 << 20)) {
    srt::SetError("BVH deeper than the query traversal stack supports (2^20 levels)");
    return SRT_ERR_LIMIT;
  }
  srt::stage::Owned<srt_query> q(new srt_query());
  q->n_bvhs = q->bvh_count = n_bvhs;
  q->first_index0 = bvhs[0].first_index;
  q->plan = srt::query::PlanStack(lay, n_tris);
  // Refill threshold ("Ray queries"): a scene the caches hold (Rubik, 74 KB) gains from
  // refilling early (surface rays 1.90 ms with 1, 1.54 with 40-56, 1.59 with 64); the 262k-triangle knot
  // (20 MB) loses (6.82 ms with 1, 7.5-7.9 with 16-64: fresh rays at the root beside deep ones touch more
  // lines per load), so its waves take new rays only when every lane is done.  SRT_QUERY_REFILL=1..64 forces it.
  const size_t scene_bytes = (lay.pairs.size() + lay.roots.size() + lay.tris.size()) * sizeof(float4);
  const char* e = std::getenv("SRT_QUERY_REFILL");
  q->refill_min = std::max(1, std::min(64, e ? std::atoi(e) : (scene_bytes < (1u << 20) ? 48 : 1)));
  e = std::getenv("SRT_QUERY_CLAIM");
  q->claim_env = e ? std::max(0, std::min(64, std::atoi(e))) : 0;
  if (int rc = q->Acquire(device, stream)) return rc;
  if (int rc = Upload(q.get(), lay, bvhs)) return rc;
  if (flags & SRT_QUERY_REFIT)
    if (int rc = srt::refit::Attach(q.get(), lay, tris, n_tris, n_verts)) return rc;
  *out = q.release();
  return SRT_OK;
}

int srt_query_create_obj(int device, void* stream, const srt_scene* s, srt_query** out) {
  return srt_query_create_obj_ex(device, stream, s, 0, out);
}

int srt_query_create_obj_ex(int device, void* stream, const srt_scene* s, uint32_t flags, srt_query** out) {
  if (!s || !out) return SRT_ERR_INVALID;
  srt::stage::SceneArrays a;
  if (int rc = srt::stage::CopyScene(s, &a)) return rc;
  return srt_query_create_ex(device, stream, a.bvhs.data(), (uint32_t)a.bvhs.size(), a.nodes.data(),
                             (uint32_t)a.nodes.size(), a.tris.data(), (uint32_t)a.tris.size(), a.verts.data(),
                             (uint32_t)a.verts.size(), flags, out);
}

int srt_query_destroy(srt_query* q) {
  if (!q) return SRT_ERR_INVALID;
  srt::stage::Destroy()(q);
  return SRT_OK;
}

int srt_query_set_bvh_count(srt_query* q, uint32_t bvh_count) {
  if (!q) return SRT_ERR_INVALID;
  q->bvh_count = bvh_count;
  return SRT_OK;
}

int srt_query_update_model_matrix(srt_query* q, uint32_t index, const float frame[16]) {
  if (!q || !frame) return SRT_ERR_INVALID;
  if (index >= q->n_bvhs) {
    srt::SetError("UpdateModelMatrix: index out of range");
    return SRT_ERR_INVALID;
  }
  STAGE_HIP_OK(hipSetDevice(q->device));
  // ordered with the queries on the stream; the 64 B leave `frame` before the call returns
  STAGE_HIP_OK(hipMemcpyAsync(q->d_frames + 16 * (size_t)index, frame, 16 * sizeof(float), hipMemcpyHostToDevice, q->stream));
  return SRT_OK;
}

int srt_query_closest(srt_query* q, const srt_ray* rays_dev, uint32_t n, srt_hit* hits_dev) {
  if (int rc = Launch<false>(q, rays_dev, n, hits_dev, nullptr)) return rc;
  // a rebuilt object holds its triangle records in the LBVH's order (include/srt_rebuild.h)
  if (n && q->rebuild && q->rebuild->count > 0) return srt::rebuild::EnqueueRemap(q, hits_dev, n);
  return SRT_OK;
}

int srt_query_occluded(srt_query* q, const srt_ray* rays_dev, uint32_t n, uint8_t* occluded_dev) {
  return Launch<true>(q, rays_dev, n, occluded_dev, nullptr);
}

int srt_query_get_int(srt_query* q, const char* name, int* v) {
  if (!q || !name || !v) return SRT_ERR_INVALID;
  const std::string n(name);
  if (n == "stack.entries") *v = q->plan.entries;
  else if (n == "stack.in_hbm") *v = q->plan.in_hbm ? 1 : 0;
  else if (n == "stack.packed") *v = q->plan.packed ? 1 : 0;
  else if (n == "launch.blocks") *v = q->last_blocks;
  else if (n == "launch.block") *v = kBlock;
  else if (n == "scratch.bytes") *v = srt::stage::SaturateInt(256 + q->plan.hbm_block_bytes * (size_t)q->stack_blocks);
  else if (n == "scene.bytes") *v = srt::stage::SaturateInt(q->scene_bytes);
  else if (n == "refill.min") *v = q->refill_min;
  else if (n == "bvh_count") *v = (int)q->bvh_count;
  else if (n == "refit") *v = q->refit ? 1 : 0;
  else if (n == "refit.heights") *v = (int)q->schedule.heights;
  else if (n == "refit.launches") *v = (int)q->schedule.launches;
  else if (n == "refit.bytes") *v = srt::stage::SaturateInt(q->refit_bytes);
  else if (n == "refit.count") *v = q->refit_count;
  else if (n == "layout.pairs") *v = srt::stage::SaturateInt(q->pairs_bytes);
  else if (n == "layout.roots") *v = srt::stage::SaturateInt(q->roots_bytes);
  else if (n == "layout.tris") *v = srt::stage::SaturateInt(q->tris_bytes);
  else if (n == "rebuild") *v = q->rebuild ? 1 : 0;
  else if (n == "rebuild.count") *v = q->rebuild ? q->rebuild->count : 0;
  else if (n == "rebuild.bytes") *v = q->rebuild ? srt::stage::SaturateInt(q->rebuild->bytes) : 0;
  else if (n == "rebuild.launches") *v = q->rebuild ? q->rebuild->launches : 0;
  else if (n == "rebuild.depth") *v = q->rebuild ? q->rebuild->depth : 0;
  else if (n == "rebuild.leaf") *v = q->rebuild ? (int)q->rebuild->max_leaf : 0;
  else if (n == "rebuild.max_leaf") *v = q->rebuild ? (int)q->rebuild->largest_leaf : 0;
  else if (n == "rebuild.pairs") *v = q->rebuild ? srt::stage::SaturateInt(q->rebuild->pairs) : 0;
  else if (n == "rebuild.leaf_bytes") *v = q->rebuild ? srt::stage::SaturateInt(q->rebuild->leaf_bytes) : 0;
  else if (n.rfind("rebuild.height.", 0) == 0) {  // pairs at one height of the last rebuild's tree, as the device counted
    char* end = nullptr;
    const unsigned long h = std::strtoul(name + 15, &end, 10);
    if (end == name + 15 || *end != '\0') return SRT_ERR_NOT_FOUND;
    *v = q->rebuild && q->rebuild->count > 0 && h < (unsigned long)srt::rebuild::kHeightBins
             ? srt::stage::SaturateInt(q->rebuild->summary[h]) : 0;
  }
  else if (n == "rebuild.models") *v = q->rebuild && q->rebuild->models ? 1 : 0;
  else if (n == "rebuild.records") *v = q->rebuild ? (int)q->rebuild->records : 0;
  else if (n == "sort.origin_bits") *v = srt::rayorder::OriginBits();
  else if (n == "sort.dir_bits") *v = srt::rayorder::DirBits();
  else if (n == "sort.bytes") *v = q->sort ? srt::stage::SaturateInt(q->sort->bytes) : 0;
  else if (n == "sort.launches") *v = q->sort ? q->sort->launches : 0;
  else if (n == "sort.count") *v = q->sort ? q->sort->count : 0;
  else return SRT_ERR_NOT_FOUND;
  return SRT_OK;
}

void* srt_query_stream(srt_query* q) { return srt::stage::StreamOf(q); }

}  // extern "C"
