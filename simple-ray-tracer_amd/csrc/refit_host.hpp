// refit_host.hpp -- host-only parts of the BVH refit (include/srt_refit.h): the refit of the std430 node
// array (srt_bvh_refit) and the schedule of the device refit, derived from query_host.hpp's Layout.  No device,
// no HIP header: tests/cpp/test_refit_host.cpp links refit_host.cpp alone.
#pragma once

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/srt_amd.h"
#include "query_host.hpp"
#include "refit_levels.hpp"

namespace srt {
namespace refit {

// The fold of include/srt_refit.h, one component.
inline float FoldMin(float m, float v) { return v < m ? v : m; }
inline float FoldMax(float m, float v) { return v > m ? v : m; }

// The leaf rule over triangles first .. first+count-1 (count >= 1, the range inside `tris`).
void LeafBox(const srt_triangle* tris, uint32_t first, uint32_t count, const srt_vertex* verts, uint32_t n_verts,
             float lo[3], float hi[3]);

// srt_bvh_refit without the error string's global: validates as query::BuildLayout does (the same messages),
// rejects a non-finite vertex position, and only then rewrites the bounds of the reached nodes.
int RefitNodes(const srt_bvh_record* bvhs, uint32_t n_bvhs, srt_bvh_node* nodes, uint32_t n_nodes,
               const srt_triangle* tris, uint32_t n_tris, const srt_vertex* verts, uint32_t n_verts, std::string* err);

// The device refit walks the pairs bottom-up by height: 0 when both slots of a pair are leaves, else 1 + the
// largest height of its internal slots' pairs.  `order` lists the pair indices by height (refit_levels.hpp); the
// tail's block then computes the roots, and `launches` always counts the triangle kernel.
struct Schedule : Levels {
  std::vector<uint32_t> order;  // n_pairs entries
};
Schedule BuildSchedule(const query::Layout& l);

}  // namespace refit
}  // namespace srt
