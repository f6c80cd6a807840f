// scene_layout.hpp -- pure host parts of the path tracer's context: validation of a caller's BVH arrays,
// the device node and triangle layouts srt_upload_scene writes, and the span-union arithmetic of the
// kernel timers.  No device, no HIP header: tests/cpp/test_scene_layout.cpp links scene_layout.cpp alone.
#pragma once

#include <cstdint>
#include <utility>
#include <vector>

#include "srt_internal.hpp"

namespace srt {

// Depth of each BVH and index validation of every node some traversal can reach (marked in `reach`).
int ValidateNodes(const srt_bvh_node* nodes, uint32_t n_nodes, uint32_t n_tris, const srt_bvh_record* bvhs,
                  uint32_t n_bvhs, int* max_depth, std::vector<std::pair<uint32_t, uint32_t>>* tri_ranges,
                  std::vector<uint8_t>* reach);

// Device node layout: pairs in the traversal's order, the top `top_depth` levels first.
bool LayoutNodes(const srt_bvh_node* nodes, uint32_t n_nodes, const srt_bvh_record* bvhs, uint32_t n_bvhs,
                 bool align, std::vector<uint32_t>* remap, uint32_t* n_slots, int top_depth = 0,
                 uint32_t* n_top_slots = nullptr);

// The slots LayoutNodes(..., top_depth) gives its top region, from its first pass alone.
bool TopRegionSlots(const srt_bvh_node* nodes, uint32_t n_nodes, const srt_bvh_record* bvhs, uint32_t n_bvhs,
                    bool align, int top_depth, uint32_t* n_top);

// Device triangle slots: one- and two-triangle leaves within one 128-B line.
bool LayoutTris(const srt_bvh_node* nodes, uint32_t n_nodes, const std::vector<uint8_t>& reach, uint32_t n_tris,
                std::vector<uint32_t>* slot, uint32_t* n_slots);

// Span records of sample launches: `ring` holds `cap` records {start, end} (100 MHz ticks), record q at
// 2 * (q % cap); `seq` records have been written so far.
bool SpanRecord(const unsigned long long* ring, unsigned long long seq, unsigned long long cap, unsigned long long q,
                unsigned long long* t0, unsigned long long* t1);
double SpanUnionMs(const unsigned long long* ring, unsigned long long seq, unsigned long long cap,
                   unsigned long long from, unsigned long long to, unsigned long long after,
                   unsigned long long* last_end);

}  // namespace srt
