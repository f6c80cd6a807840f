// rebuild.hip -- the device rebuild of include/srt_rebuild.h, srt_rebuild_leaf.h and srt_rebuild_models.h: the rebuild
// data of a query object (Enable, SetLeaf), and one Rebuild -- the launches of rebuild.hpp's kernels around hipcub's
// radix sort, the one readback, the new schedule and stack plan, the refit that fills the boxes -- and the hit remap.
// The case enters Rebuild as data: the records (one: the scene box and a 32-bit sort; several: a box per record and a
// 64-bit (record, key) sort, and the SEG instances of the kernels), max_leaf (above 1 a range kernel, hipcub's scan and
// an emit kernel stand in the hierarchy kernel's place), and what SegmentShape says of the segments.  A translation
// unit of its own beside query.hip and refit.hip.
#include <hip/hip_runtime.h>
#include <hipcub/device/device_radix_sort.hpp>
#include <hipcub/device/device_scan.hpp>

#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "../../include/srt_rebuild.h"
#include "../../include/srt_rebuild_leaf.h"
#include "../../include/srt_rebuild_models.h"
#include "query_object.hpp"
#include "rebuild.hpp"
#include "rebuild_host.hpp"
#include "stage.hpp"

namespace srt {
namespace rebuild {

namespace {

constexpr int kKeyBits = 30;

uint32_t Blocks(uint32_t n) { return (n + kBlock - 1) / kBlock; }

int RecordBits(uint32_t records) {
  int bits = 1;
  while (bits < 32 && (1ull << bits) < records) ++bits;
  return bits;
}

// One record: the 30 key bits.  Several: the (record, key) sort over bits [0, 32 + the records' bits) of the 64-bit
// keys.  Stable, as every radix sort is.
hipError_t Sort(State& st, uint32_t n, hipStream_t stream, void* temp, size_t& temp_bytes) {
  if (st.records > 1)
    return hipcub::DeviceRadixSort::SortPairs(temp, temp_bytes, (const uint64_t*)st.d_keys64_in.get(), st.d_keys64.get(),
                                              (const uint32_t*)st.d_vals_in.get(), st.d_order.get(), n, 0,
                                              32 + RecordBits(st.records), stream);
  return hipcub::DeviceRadixSort::SortPairs(temp, temp_bytes, (const uint32_t*)st.d_keys_in.get(), st.d_keys.get(),
                                            (const uint32_t*)st.d_vals_in.get(), st.d_order.get(), n, 0, kKeyBits, stream);
}

// d_zeroed: counts, cursor, the arrival words, and with several records their boxes.
size_t ZeroedWords(uint32_t n, uint32_t records) {
  return 2 * (size_t)kHeightBins + (n - 1) + (records > 1 ? 8 * (size_t)records : 0);
}

// An allocation the object reports: `total` is rebuild.bytes or rebuild.leaf_bytes.
template <class T>
hipError_t Alloc(stage::DevPtr<T>& p, size_t bytes, size_t& total) {
  total += bytes;
  return p.Alloc(bytes);
}

// rank = the exclusive sum of the n survival flags (the last is 0, so rank[n - 1] is the number of survivors)
hipError_t Scan(const uint32_t* flags, uint32_t* rank, uint32_t n, hipStream_t stream, void* temp, size_t& temp_bytes) {
  return hipcub::DeviceScan::ExclusiveSum(temp, temp_bytes, flags, rank, (int)n, stream);
}

// The end of every rebuild, after its one synchronisation: the schedule from the counts per height, the object's
// description of the tree built (m pairs in the first `extent` slots of the pair array), the stack plan, the refit.
int Adopt(srt_query* q, const srt_vertex* verts_dev, int launches, uint32_t m, uint32_t extent, uint32_t largest,
          bool summary_valid) {
  State& st = *q->rebuild;
  const uint32_t n = q->n_tris;
  hipStream_t s = q->stream;
  refit::Schedule sched;
  if (!summary_valid || !ScheduleFromCounts(st.summary, kHeightBins, m, &sched)) {
    srt::SetError("srt_query_rebuild: the device hierarchy is not a tree over every triangle (non-finite vertices?)");
    return SRT_ERR_STATE;
  }
  st.summary[kHeightBins] = sched.heights;
  st.summary[kHeightBins + 1] = m;
  // the object describes the tree built: the first `extent` pairs of the array's n - 1
  const size_t pb = 4 * sizeof(float4) * (size_t)(extent ? extent : 1u), tb = sizeof(uint4) * (size_t)n;
  q->scene_bytes = q->scene_bytes - q->pairs_bytes + pb;
  q->pairs_bytes = pb;
  q->n_pairs = m;
  q->refit_bytes = tb + sizeof(uint32_t) * ((size_t)m + kHeightBins + 1);
  st.tail_first.assign(sched.first.begin() + sched.tail_begin, sched.first.end());
  STAGE_HIP_OK(hipMemcpyAsync(q->d_schedule + m, st.tail_first.data(), sizeof(uint32_t) * st.tail_first.size(),
                              hipMemcpyHostToDevice, s));
  q->schedule = std::move(sched);
  // the stack plan of the new tree: its largest leaf, depth == heights
  query::Layout shape;
  shape.n_pairs = extent;
  shape.max_leaf = largest;
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
  st.pairs = m;
  st.largest_leaf = largest;
  ++st.count;
  return SRT_OK;
}

}  // namespace

// The rebuild data of an object of q->n_bvhs records.  With two or more, first the owners from the object's own pairs and
// roots, and beside the common arrays 64-bit sort keys, the per-record boxes behind the arrival words, and the segment
// arrays; with one, the segment is [0, n) and the arrays are the scene box's and the 32-bit keys'.
int Enable(srt_query* q) {
  STAGE_HIP_OK(hipSetDevice(q->device));
  const uint32_t n = q->n_tris, n_pairs = n - 1, records = q->n_bvhs;
  const bool seg = records > 1;
  std::vector<uint32_t> owner(n, 0u);
  std::string err;
  if (seg) {
    STAGE_HIP_OK(hipStreamSynchronize(q->stream));
    std::vector<query::F4> pairs(q->pairs_bytes / sizeof(query::F4)), roots(q->roots_bytes / sizeof(query::F4));
    STAGE_HIP_OK(hipMemcpy(pairs.data(), q->d_pairs, q->pairs_bytes, hipMemcpyDeviceToHost));
    STAGE_HIP_OK(hipMemcpy(roots.data(), q->d_roots, q->roots_bytes, hipMemcpyDeviceToHost));
    if (roots.size() < 2 * ((size_t)records + 1) || pairs.size() < 4 * (size_t)q->n_pairs) return SRT_ERR_STATE;
    if (int rc = OwnersFromLayout(pairs.data(), q->n_pairs, roots.data(), records, n, owner.data(), &err)) {
      srt::SetError(err);
      return rc;
    }
  }
  std::unique_ptr<State> st(new State());
  st->records = records;
  st->segments = SegmentsOf(owner.data(), n, records);
  if (int rc = CheckSegments(st->segments, &err)) {
    srt::SetError(err);
    return rc;
  }
  const size_t per_tri = sizeof(uint32_t) * (size_t)n, per_pair = sizeof(uint32_t) * (size_t)(n_pairs ? n_pairs : 1u);
  const size_t seg_bytes = sizeof(uint2) * (size_t)records;
  size_t& bytes = st->bytes;
  STAGE_HIP_OK(Alloc(st->d_pairs, 4 * sizeof(float4) * (size_t)(n_pairs ? n_pairs : 1u), bytes));
  STAGE_HIP_OK(Alloc(st->d_triples, sizeof(uint4) * (size_t)n, bytes));
  STAGE_HIP_OK(Alloc(st->d_schedule, sizeof(uint32_t) * ((size_t)n_pairs + kHeightBins + 1), bytes));
  STAGE_HIP_OK(Alloc(st->d_vals_in, per_tri, bytes));
  STAGE_HIP_OK(Alloc(st->d_keys, per_tri, bytes));
  STAGE_HIP_OK(Alloc(st->d_order, per_tri, bytes));
  STAGE_HIP_OK(Alloc(st->d_parent, 2 * per_tri, bytes));
  STAGE_HIP_OK(Alloc(st->d_height, per_pair, bytes));
  STAGE_HIP_OK(Alloc(st->d_zeroed, sizeof(uint32_t) * ZeroedWords(n, records), bytes));
  if (seg) {
    STAGE_HIP_OK(Alloc(st->d_keys64_in, 2 * per_tri, bytes));
    STAGE_HIP_OK(Alloc(st->d_keys64, 2 * per_tri, bytes));
    STAGE_HIP_OK(Alloc(st->d_owner, per_tri, bytes));
    STAGE_HIP_OK(Alloc(st->d_pos_rec, per_tri, bytes));
    STAGE_HIP_OK(Alloc(st->d_seg, seg_bytes, bytes));
  } else {
    STAGE_HIP_OK(Alloc(st->d_keys_in, per_tri, bytes));
    STAGE_HIP_OK(Alloc(st->d_box, sizeof(float) * 8 * (1 + (size_t)kBoxBlocks), bytes));
  }
  size_t temp = 0;
  STAGE_HIP_OK(Sort(*st, n, q->stream, nullptr, temp));  // the size only
  st->temp_bytes = temp ? temp : 16;
  STAGE_HIP_OK(Alloc(st->d_temp, st->temp_bytes, bytes));
  std::vector<uint32_t> pos_rec;
  std::vector<uint2> segs;
  if (seg) {
    pos_rec.resize(n);
    segs.resize(records);
    for (uint32_t r = 0; r < records; ++r) {
      segs[r] = make_uint2(st->segments.first[r], st->segments.count[r]);
      for (uint32_t k = 0; k < st->segments.count[r]; ++k) pos_rec[st->segments.first[r] + k] = r;
    }
    STAGE_HIP_OK(hipMemcpyAsync(st->d_owner, owner.data(), per_tri, hipMemcpyHostToDevice, q->stream));
    STAGE_HIP_OK(hipMemcpyAsync(st->d_pos_rec, pos_rec.data(), per_tri, hipMemcpyHostToDevice, q->stream));
    STAGE_HIP_OK(hipMemcpyAsync(st->d_seg, segs.data(), seg_bytes, hipMemcpyHostToDevice, q->stream));
  }
  // one triangle: the order is the identity for good (its rebuild is a refit)
  STAGE_HIP_OK(hipMemsetAsync(st->d_order, 0, per_tri, q->stream));
  STAGE_HIP_OK(hipStreamSynchronize(q->stream));  // the host arrays go out of scope
  q->rebuild = std::move(st);
  return SRT_OK;
}

// What the collapse adds on the device, at the first max_leaf above 1 (a mesh of one triangle never needs it).
int SetLeaf(srt_query* q, uint32_t max_leaf) {
  State& st = *q->rebuild;
  const uint32_t n = q->n_tris;
  if (max_leaf > 1 && n > 1 && !st.d_flags) {
    STAGE_HIP_OK(hipSetDevice(q->device));
    stage::DevPtr<uint4> split;
    stage::DevPtr<uint32_t> flags, rank, leafsum;
    stage::DevPtr<uint8_t> scan_temp;
    const size_t per_tri = sizeof(uint32_t) * (size_t)n;
    size_t bytes = 0;
    STAGE_HIP_OK(Alloc(split, sizeof(uint4) * (size_t)(n - 1), bytes));
    STAGE_HIP_OK(Alloc(flags, per_tri, bytes));
    STAGE_HIP_OK(Alloc(rank, per_tri, bytes));
    STAGE_HIP_OK(Alloc(leafsum, 2 * sizeof(uint32_t), bytes));
    size_t temp = 0;
    STAGE_HIP_OK(Scan(flags, rank, n, q->stream, nullptr, temp));  // the size only: nothing is enqueued
    temp = temp ? temp : 16;
    STAGE_HIP_OK(Alloc(scan_temp, temp, bytes));
    // (every allocation succeeded: only now does the state change)
    st.scan_temp_bytes = temp;
    st.d_flags = std::move(flags);
    st.d_rank = std::move(rank);
    st.d_split = std::move(split);
    st.d_leafsum = std::move(leafsum);
    st.d_scan_temp = std::move(scan_temp);
    st.leaf_bytes = bytes;
  }
  st.max_leaf = max_leaf;
  return SRT_OK;
}

namespace {

// The kernels' view of the state and the object: every array the case has (the others stay null).
BParams Bind(const State& st, const srt_query* q, const srt_vertex* verts_dev) {
  const uint32_t n = q->n_tris;
  BParams bp;
  std::memset(&bp, 0, sizeof bp);
  bp.pairs = q->d_pairs;
  bp.roots = q->d_roots;
  bp.triples0 = st.d_triples;
  bp.triples = q->d_triples;
  bp.verts = reinterpret_cast<const float4*>(verts_dev);
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
  bp.n_records = st.records;
  if (st.records > 1) {
    bp.owner = st.d_owner;
    bp.pos_rec = st.d_pos_rec;
    bp.seg = st.d_seg;
    bp.seg_box = bp.arrive + (n - 1);
    bp.keys64_in = st.d_keys64_in;
    bp.keys64 = st.d_keys64;
    bp.keys_out = st.d_keys;
  } else {
    bp.box = st.d_box;
    bp.box_partial = st.d_box + 8;
    bp.keys_in = st.d_keys_in;
    bp.box_blocks = Blocks(n) < kBoxBlocks ? Blocks(n) : kBoxBlocks;
  }
  if (st.max_leaf > 1) {
    bp.split = st.d_split;
    bp.flags = st.d_flags;
    bp.rank = st.d_rank;
    bp.leafsum = st.d_leafsum;
    bp.max_leaf = st.max_leaf;
  }
  return bp;
}

}  // namespace

int Rebuild(srt_query* q, const srt_vertex* verts_dev) {
  STAGE_HIP_OK(hipSetDevice(q->device));
  State& st = *q->rebuild;
  const uint32_t n = q->n_tris;
  if (n == 1) {  // a leaf root: nothing to sort, the refit is the rebuild
    if (int rc = refit::Enqueue(q, verts_dev)) return rc;
    st.launches = (int)q->schedule.launches;
    st.depth = 0;
    st.pairs = 0;
    st.largest_leaf = 1;
    ++st.count;
    return SRT_OK;
  }
  const uint32_t n_pairs = n - 1;      // the pair array's capacity
  const uint32_t max_leaf = st.max_leaf;
  const bool seg = st.records > 1;
  const bool collapse = max_leaf > 1;  // rules 4a-4c; false: exactly srt_rebuild.h's launches
  uint32_t karras_pairs = 0, root_leaf = 0;  // what the segments say before the device ran
  SegmentShape(st.segments, max_leaf, &karras_pairs, &root_leaf);
  // one record of n <= max_leaf triangles: the sort, the root, the refit.  (Several records that are all leaf roots go
  // through the collapse's kernels, which write every root; their m is 0 too.)
  const bool root_only = !seg && karras_pairs == 0;
  const bool emitted = collapse && !root_only;  // leafsum is this rebuild's
  const bool first_time = st.count == 0;
  if (first_time) {
    // the LBVH's arrays take the object's place; the state keeps the creation-order triples for every later
    // sort, and the replaced tree's pairs and schedule until the synchronisation below
    std::swap(st.d_pairs, q->d_pairs);
    std::swap(st.d_triples, q->d_triples);
    std::swap(st.d_schedule, q->d_schedule);
  }
  const BParams bp = Bind(st, q, verts_dev);
  hipStream_t s = q->stream;
  int launches = 0;
  auto launch = [&](void (*kernel)(BParams), uint32_t blocks) {
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(kBlock), 0, s, bp);
    ++launches;
    return hipGetLastError();
  };
  STAGE_HIP_OK(hipMemsetAsync(st.d_zeroed, 0, sizeof(uint32_t) * ZeroedWords(n, st.records), s));
  if (seg) {
    STAGE_HIP_OK(launch(seg_box_kernel, Blocks(n)));
  } else {
    STAGE_HIP_OK(launch(box_partial_kernel, bp.box_blocks));
    STAGE_HIP_OK(launch(box_final_kernel, 1));
  }
  STAGE_HIP_OK(launch(seg ? keys_kernel<true> : keys_kernel<false>, Blocks(n)));
  size_t temp = st.temp_bytes;
  STAGE_HIP_OK(Sort(st, n, s, st.d_temp, temp));
  ++launches;  // (the sort's own launches are hipcub's business: counted as one)
  STAGE_HIP_OK(launch(seg ? permute_kernel<true> : permute_kernel<false>, Blocks(n)));
  if (root_only) {
    STAGE_HIP_OK(launch(root_leaf_kernel, 1));
  } else {
    if (collapse) {
      STAGE_HIP_OK(launch(seg ? range_kernel<true> : range_kernel<false>, Blocks(n)));
      size_t scan_temp = st.scan_temp_bytes;
      STAGE_HIP_OK(Scan(st.d_flags, st.d_rank, n, s, st.d_scan_temp, scan_temp));
      ++launches;  // (hipcub's business again: counted as one)
      STAGE_HIP_OK(launch(seg ? emit_kernel<true> : emit_kernel<false>, Blocks(n)));
    } else {
      STAGE_HIP_OK(launch(seg ? karras_kernel<true> : karras_kernel<false>, Blocks(n)));
    }
    STAGE_HIP_OK(launch(collapse ? climb_kernel<true> : climb_kernel<false>, Blocks(n)));
    STAGE_HIP_OK(launch(collapse ? (seg ? schedule_kernel<true, true> : schedule_kernel<true, false>)
                                 : (seg ? schedule_kernel<false, true> : schedule_kernel<false, false>),
                        Blocks(n_pairs)));
  }
  if (karras_pairs == 0 && collapse)  // no pair at all: pair 0, which srt_query_copy_layout still copies, keeps nothing
    STAGE_HIP_OK(hipMemsetAsync(q->d_pairs, 0, 4 * sizeof(float4), s));
  // the one synchronisation: the pair counts per height, and of a collapsed tree its pairs and its largest leaf
  STAGE_HIP_OK(hipMemcpyAsync(st.summary, st.d_zeroed, sizeof(uint32_t) * kHeightBins, hipMemcpyDeviceToHost, s));
  if (emitted) STAGE_HIP_OK(hipMemcpyAsync(st.leaf_summary, st.d_leafsum, sizeof st.leaf_summary, hipMemcpyDeviceToHost, s));
  STAGE_HIP_OK(hipStreamSynchronize(s));
  if (first_time) {  // nothing enqueued reads the replaced tree any more
    st.d_pairs.Free();
    st.d_schedule.Free();
  }
  // without the emit kernel nothing was read back: m and the largest leaf are the segments' (a leaf root: 0 and n)
  const uint32_t m = emitted ? st.leaf_summary[0] : karras_pairs;
  const uint32_t device_largest = emitted ? st.leaf_summary[1] : (karras_pairs ? 1u : 0u);
  const uint32_t largest = device_largest > root_leaf ? device_largest : root_leaf;
  const bool valid = !emitted || ModelsSummaryValid(m, device_largest, karras_pairs, max_leaf);
  return Adopt(q, verts_dev, launches, m, collapse ? m : n_pairs, largest, valid);
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

int srt_rebuild_leaf_abi_version(void) { return SRT_REBUILD_LEAF_ABI_VERSION; }

int srt_bvh_build_lbvh_leaf(const srt_triangle* tris, uint32_t n_tris, const srt_vertex* verts, uint32_t n_verts,
                            uint32_t max_leaf, srt_bvh_node* nodes_out, uint32_t* n_nodes_out, srt_triangle* tris_out,
                            uint32_t* order_out) {
  std::string err;
  const int rc = srt::rebuild::BuildLBVHLeaf(tris, n_tris, verts, n_verts, max_leaf, nodes_out, n_nodes_out, tris_out,
                                             order_out, &err);
  if (rc) srt::SetError(err);
  return rc;
}

int srt_query_set_rebuild_leaf(srt_query* q, uint32_t max_leaf) {
  std::string err;
  if (int rc = srt::rebuild::CheckSetLeaf(q != nullptr, q && q->rebuild, max_leaf, &err)) {
    srt::SetError(err);
    return rc;
  }
  return srt::rebuild::SetLeaf(q, max_leaf);
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

int srt_rebuild_models_abi_version(void) { return SRT_REBUILD_MODELS_ABI_VERSION; }

int srt_bvh_build_lbvh_models(const srt_bvh_record* bvhs, uint32_t n_bvhs, const srt_bvh_node* nodes, uint32_t n_nodes,
                              const srt_triangle* tris, uint32_t n_tris, const srt_vertex* verts, uint32_t n_verts,
                              uint32_t max_leaf, srt_bvh_record* bvhs_out, srt_bvh_node* nodes_out, uint32_t* n_nodes_out,
                              srt_triangle* tris_out, uint32_t* order_out) {
  std::string err;
  const int rc = srt::rebuild::BuildLBVHModels(bvhs, n_bvhs, nodes, n_nodes, tris, n_tris, verts, n_verts, max_leaf, bvhs_out,
                                               nodes_out, n_nodes_out, tris_out, order_out, &err);
  if (rc) srt::SetError(err);
  return rc;
}

int srt_query_enable_rebuild_models(srt_query* q) {
  std::string err;
  if (int rc = srt::rebuild::CheckEnableModels(q != nullptr, q && q->refit, q ? q->first_index0 : 0, q ? q->n_tris : 0, &err)) {
    srt::SetError(err);
    return rc;
  }
  if (q->rebuild) return SRT_OK;
  // (one record owns every triangle its root reaches, and the layout holds no other: srt_rebuild.h's object exactly)
  if (int rc = srt::rebuild::Enable(q)) return rc;
  q->rebuild->models = true;
  return SRT_OK;
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
