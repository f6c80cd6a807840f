// query_object.hpp -- the srt_query object, shared by the two translation units that work on it: query.hip
// (creation, the queries) and refit.hip (include/srt_refit.h: the device refit and the layout readback).
#pragma once

#include <cstddef>
#include <cstdint>
#include <memory>
#include <vector>

#include "../../include/srt_refit.h"
#include "query_host.hpp"
#include "rebuild_host.hpp"
#include "refit_host.hpp"
#include "stage.hpp"

namespace srt {
namespace rebuild {

// What srt_query_enable_rebuild adds to an object (rebuild.hip, include/srt_rebuild.h).  Until the first rebuild
// d_pairs / d_triples / d_schedule are the LBVH's arrays-to-be; that rebuild exchanges them with the object's,
// and they then hold the creation-order index triples (kept: every rebuild sorts from them) and the replaced
// tree's pairs and schedule (freed after that rebuild's synchronisation).
//
// Which arrays exist (the others stay null):
//   always                    d_pairs, d_triples, d_schedule, d_vals_in, d_keys, d_order, d_temp, d_parent, d_height,
//                             d_zeroed
//   one record                d_keys_in (the 32-bit sort's input; d_keys is its output), d_box
//   two records or more       d_keys64_in, d_keys64 (the 64-bit sort; d_keys holds the sorted low dwords), d_owner,
//                             d_pos_rec, d_seg; the records' boxes follow the arrival words in d_zeroed
//   from the first max_leaf   d_split, d_flags, d_rank, d_leafsum, d_scan_temp (counted in leaf_bytes, not in bytes)
//   above 1, and n > 1
struct State {
  stage::DevPtr<float4> d_pairs;
  stage::DevPtr<uint4> d_triples;
  stage::DevPtr<uint32_t> d_schedule;
  stage::DevPtr<uint32_t> d_keys_in, d_vals_in, d_keys, d_order;  // the sort's input and output
  stage::DevPtr<uint8_t> d_temp;                                  // its temporary storage
  size_t temp_bytes = 0;
  stage::DevPtr<uint32_t> d_parent, d_height;
  stage::DevPtr<uint32_t> d_zeroed;  // zeroed by every rebuild: counts, cursor, the arrival words, the records' boxes
  stage::DevPtr<float> d_box;        // the scene box, then the partial boxes
  size_t bytes = 0;
  int count = 0, launches = 0, depth = 0;
  uint32_t summary[kSummaryInts] = {};
  std::vector<uint32_t> tail_first;  // host copy of the tail's level offsets while their upload is in flight
  // srt_query_set_rebuild_leaf (include/srt_rebuild_leaf.h); allocated by the first value above 1
  uint32_t max_leaf = 1;             // the setting, for the next rebuild
  stage::DevPtr<uint4> d_split;      // n - 1: first, last, gamma, survives
  stage::DevPtr<uint32_t> d_flags, d_rank;  // n each: the scan's input and output
  stage::DevPtr<uint32_t> d_leafsum;        // m, the largest leaf count
  stage::DevPtr<uint8_t> d_scan_temp;
  size_t scan_temp_bytes = 0, leaf_bytes = 0;
  uint32_t leaf_summary[2] = {};     // what the last collapsed rebuild read back from d_leafsum
  uint32_t pairs = 0, largest_leaf = 0;  // of the last rebuild's tree
  // include/srt_rebuild_models.h
  bool models = false;                       // enabled by srt_query_enable_rebuild_models
  uint32_t records = 1;
  Segments segments;                         // s_r, n_r: fixed when enabled (one record: 0, n)
  stage::DevPtr<uint32_t> d_owner, d_pos_rec;  // n each: creation index -> record, position -> record
  stage::DevPtr<uint2> d_seg;                  // per record
  stage::DevPtr<uint64_t> d_keys64_in, d_keys64;
};

}  // namespace rebuild

namespace rayorder {

// What the first sorted call adds to an object (query_sort.hip, include/srt_query_sort.h), grown only when n grows.
struct State {
  stage::DevPtr<uint32_t> d_pairs;   // 4 arrays of `capacity` dwords: keys_in, order_in, keys (sorted), order (sorted)
  stage::DevPtr<uint8_t> d_temp;     // the sort's temporary storage
  stage::DevPtr<uint32_t> d_words;   // the six bounds words (ray_order_rule.hpp)
  uint32_t capacity = 0;
  size_t temp_bytes = 0, bytes = 0;  // bytes: everything above
  uint32_t last_n = 0;               // of the last sorted call
  int launches = 0, count = 0;
  uint32_t* keys_in() const { return d_pairs.get(); }
  uint32_t* order_in() const { return d_pairs.get() + capacity; }
  uint32_t* keys() const { return d_pairs.get() + 2 * (size_t)capacity; }
  uint32_t* order() const { return d_pairs.get() + 3 * (size_t)capacity; }
};

}  // namespace rayorder
}  // namespace srt

struct srt_query : srt::stage::Stage {
  srt::stage::DevPtr<float4> d_pairs, d_roots, d_tris;
  srt::stage::DevPtr<float> d_frames;
  srt::stage::DevPtr<uint32_t> d_ctr;
  srt::stage::DevPtr<uint32_t> d_stack;  // HBM stacks of `stack_blocks` blocks (deep trees only)
  int stack_blocks = 0;
  size_t scene_bytes = 0;
  size_t pairs_bytes = 0, roots_bytes = 0, tris_bytes = 0;  // of d_pairs / d_roots / d_tris
  uint32_t n_bvhs = 0, bvh_count = 0;
  srt::query::StackPlan plan;
  int max_blocks[2] = {0, 0};  // persistent grid of the closest / any instance
  int max_blocks_sorted[2] = {0, 0};  // of their ORDER twins
  int refill_min = 0, claim_env = 0;
  int last_blocks = 0;
  // SRT_QUERY_REFIT only (refit.hip); nothing here is allocated without the flag
  bool refit = false;
  srt::stage::DevPtr<uint4> d_triples;     // srt_triangle records: v0, v1, v2, material
  srt::stage::DevPtr<uint32_t> d_schedule; // Schedule::order, then the tail's level offsets
  srt::refit::Schedule schedule;           // (`order` is dropped after the upload)
  uint32_t n_pairs = 0, n_tris = 0, n_verts = 0;
  size_t refit_bytes = 0;
  int refit_count = 0;
  // srt_query_enable_rebuild only (rebuild.hip); null otherwise
  uint32_t first_index0 = 0;  // of BVH record 0
  int cu_count = 0;
  std::unique_ptr<srt::rebuild::State> rebuild;
  // the first srt_query_*_sorted call only (query_sort.hip); null otherwise
  std::unique_ptr<srt::rayorder::State> sort;
};

namespace srt {
namespace query {

// The persistent grids of the two kernel instances q->plan selects (query.hip; at creation, and again when a
// rebuild changes the plan).
int PlanGrid(srt_query* q);

// srt_query_closest (any: srt_query_occluded) with its argument checks, on q->stream.  `order` null: the rays in the
// caller's order; else the device permutation of 0 .. n-1 the launch claims through (query.hip).
int EnqueueTrace(srt_query* q, bool any, const srt_ray* rays, uint32_t n, void* out, const uint32_t* order);

}  // namespace query

namespace refit {

// Uploads the refit data of a query object created with SRT_QUERY_REFIT (on q->stream; synchronises).
int Attach(srt_query* q, const query::Layout& lay, const srt_triangle* tris, uint32_t n_tris, uint32_t n_verts);

// srt_query_refit after its argument checks: the launches, on q->stream.
int Enqueue(srt_query* q, const srt_vertex* verts_dev);

}  // namespace refit

namespace rebuild {

// The launch srt_query_closest adds on a rebuilt object: hits_dev[i].triangle, a position, becomes the creation index.
int EnqueueRemap(srt_query* q, srt_hit* hits_dev, uint32_t n);

}  // namespace rebuild
}  // namespace srt
