// query_object.hpp -- the srt_query object, shared by the two translation units that work on it: query.hip
// (creation, the queries) and refit.hip (include/srt_refit.h: the device refit and the layout readback).
#pragma once

#include <cstddef>
#include <cstdint>

#include "../../include/srt_refit.h"
#include "query_host.hpp"
#include "refit_host.hpp"
#include "stage.hpp"

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
};

namespace srt {
namespace refit {

// Uploads the refit data of a query object created with SRT_QUERY_REFIT (on q->stream; synchronises).
int Attach(srt_query* q, const query::Layout& lay, const srt_triangle* tris, uint32_t n_tris, uint32_t n_verts);

}  // namespace refit
}  // namespace srt
