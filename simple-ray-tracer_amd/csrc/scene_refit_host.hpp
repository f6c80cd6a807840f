// scene_refit_host.hpp -- host-only parts of the path tracer's scene refit (include/srt_scene_refit.h): the refit
// schedule over the device node layout and the per-triangle index records.  No device, no HIP header:
// tests/cpp/test_scene_refit_host.cpp links scene_refit_host.cpp alone.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/srt_amd.h"
#include "refit_levels.hpp"

namespace srt {
namespace scene_refit {

using refit::kBlock;

// One node to refit: its slot of the device node array and, for a leaf, the leaf's first input triangle (the
// fold walks the input order; the record itself holds the triangle's slot).
struct Entry {
  uint32_t slot, tri;
};

// The nodes go bottom-up by height: 0 for a leaf, else 1 + the larger height of the two children.  `order`
// lists the reached slots by height, ascending slot inside one (refit_levels.hpp); `launches` counts the triangle
// kernel only when there are triangles.
struct Schedule : refit::Levels {
  std::vector<Entry> order;
};

// `ref` / `cnt`: the .w fields of the n_slots records of the device node array (scene_image.hpp: an internal
// record's children are slots (ref | ref_or) and the next; a leaf's ref is its first triangle slot).  Every slot
// some root reaches is scheduled once, however many roots or parents reach it; no other slot appears.
// `tri_of_slot` (may be null: the identity) maps a triangle slot back to the input triangle.  False, with *out
// unspecified, for records no upload produces: a child, root or triangle slot out of range, or a cycle.
bool BuildSchedule(const uint32_t* ref, const uint32_t* cnt, uint32_t n_slots, uint32_t ref_or, const uint32_t* roots,
                   uint32_t n_roots, const uint32_t* tri_of_slot, uint32_t n_tri_slots, uint32_t n_tris, Schedule* out);

// Per input triangle 4 dwords: v0, v1, v2 and the triangle's slot (`tri_slot` null: the identity).
std::vector<uint32_t> BuildTriples(const srt_triangle* tris, uint32_t n_tris, const uint32_t* tri_slot);

}  // namespace scene_refit
}  // namespace srt
