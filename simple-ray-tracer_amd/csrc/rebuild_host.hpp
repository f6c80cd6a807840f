// rebuild_host.hpp -- host-only parts of the device rebuild (include/srt_rebuild.h, include/srt_rebuild_leaf.h and, at
// the end, include/srt_rebuild_models.h: the owners, the segments and the mirror for several BVH records): the
// host mirror of the LBVH (srt_bvh_build_lbvh, srt_bvh_build_lbvh_leaf), the argument contract of the object calls, and
// the refit schedule and depth from the pair counts per height the device reports.  No device, no HIP header:
// tests/cpp/test_rebuild_host.cpp and tests/cpp/test_rebuild_leaf_host.cpp link rebuild_host.cpp and refit_host.cpp
// alone.
#pragma once

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/srt_amd.h"
#include "rebuild_rule.hpp"
#include "refit_host.hpp"

namespace srt {
namespace rebuild {

constexpr int kSummaryInts = kHeightBins + 2;  // what a rebuild reads back: the counts, the heights, the pairs

// Rule 1 and 2: the scene box and the key of every triangle, in input order.
void SceneBox(const srt_triangle* tris, uint32_t n_tris, const srt_vertex* verts, uint32_t n_verts, float lo[3], float hi[3]);
void Keys(const srt_triangle* tris, uint32_t n_tris, const srt_vertex* verts, uint32_t n_verts, uint32_t* keys);

// ceil(log2 n) + 30: the depth no tree of the rule exceeds (n >= 1).
int DepthBound(uint32_t n_tris);

// srt_bvh_build_lbvh without the error string's global.
int BuildLBVH(const srt_triangle* tris, uint32_t n_tris, const srt_vertex* verts, uint32_t n_verts, srt_bvh_node* nodes_out,
              srt_triangle* tris_out, uint32_t* order_out, std::string* err);

// srt_bvh_build_lbvh_leaf (include/srt_rebuild_leaf.h) without the error string's global: rules 4a-4c on the same
// keys, order and hierarchy.  Writes 2m + 1 nodes and that count; BuildLBVH is this with max_leaf == 1.
int BuildLBVHLeaf(const srt_triangle* tris, uint32_t n_tris, const srt_vertex* verts, uint32_t n_verts, uint32_t max_leaf,
                  srt_bvh_node* nodes_out, uint32_t* n_nodes_out, srt_triangle* tris_out, uint32_t* order_out, std::string* err);

// The argument contract, before any device is touched.  `refit` / `enabled`: what the object was created with
// and whether srt_query_enable_rebuild ran; first_index: of BVH record 0.
int CheckEnable(bool have_object, bool refit, uint32_t n_bvhs, uint32_t first_index, uint32_t n_tris, std::string* err);
int CheckRebuild(bool have_object, bool refit, bool enabled, const void* verts_dev, uint32_t n_verts, uint32_t want_verts,
                 std::string* err);
int CheckSetLeaf(bool have_object, bool enabled, uint32_t max_leaf, std::string* err);

// The schedule refit::BuildSchedule would make of a tree with counts[h] pairs at height h (`order` stays empty:
// the device wrote it).  false when the counts do not add up to n_pairs -- the pair count the caller has, n - 1 or
// the collapsed tree's m as the device reported it -- or a level under the last is empty.
bool ScheduleFromCounts(const uint32_t* counts, int n_counts, uint32_t n_pairs, refit::Schedule* out);

// -- include/srt_rebuild_models.h -----------------------------------------------------------------------------------------
// The owner of every triangle: the record whose root reaches it.  From the std430 arrays (the mirror) and from a query
// object's layout as query_host.hpp describes it (pairs: 4 F4 per pair, roots: 2 F4 per record; what the object reads
// back when the rebuild is enabled).  Both refuse a reference out of range, a node or pair reached twice, and a
// triangle that belongs to no record or to more than one; owner has n_tris entries.
int OwnersFromNodes(const srt_bvh_record* bvhs, uint32_t n_bvhs, const srt_bvh_node* nodes, uint32_t n_nodes, uint32_t n_tris,
                    uint32_t* owner, std::string* err);
int OwnersFromLayout(const query::F4* pairs, uint32_t n_pairs, const query::F4* roots, uint32_t n_bvhs, uint32_t n_tris,
                     uint32_t* owner, std::string* err);

// The segments of the (record, key) order: first[r] = s_r and count[r] = n_r from the owners.
struct Segments {
  std::vector<uint32_t> first, count;
};
Segments SegmentsOf(const uint32_t* owner, uint32_t n_tris, uint32_t n_bvhs);

// A record without a triangle is refused (SRT_ERR_INVALID, "every BVH record must own at least one triangle").  A walk
// that succeeded cannot leave one -- every root is a leaf of one triangle or more, or reaches one -- so this guards the
// segment arithmetic, not a case a scene can have.
int CheckSegments(const Segments& seg, std::string* err);

// What a rebuild with `max_leaf` can say of these segments before the device ran: the pairs of Karras' hierarchies that
// exist (records above max_leaf: n_r - 1 each), and the largest leaf root.
void SegmentShape(const Segments& seg, uint32_t max_leaf, uint32_t* karras_pairs, uint32_t* largest_root_leaf);

// srt_bvh_build_lbvh_models without the error string's global.
int BuildLBVHModels(const srt_bvh_record* bvhs, uint32_t n_bvhs, const srt_bvh_node* nodes, uint32_t n_nodes,
                    const srt_triangle* tris, uint32_t n_tris, const srt_vertex* verts, uint32_t n_verts, uint32_t max_leaf,
                    srt_bvh_record* bvhs_out, srt_bvh_node* nodes_out, uint32_t* n_nodes_out, srt_triangle* tris_out,
                    uint32_t* order_out, std::string* err);

// srt_query_enable_rebuild_models' contract before any device is touched (the owners come after it).
int CheckEnableModels(bool have_object, bool refit, uint32_t first_index, uint32_t n_tris, std::string* err);

// What a collapsed rebuild reads back beside the counts, checked before anything is planned from it: m is 0 exactly when
// Karras' hierarchies hold no pair (every record a leaf root) and at most the pairs they hold, and with a pair the largest
// leaf is in [1, max_leaf].  One record of n > max_leaf triangles: karras_pairs == n - 1, so 1 <= m <= n - 1.
bool ModelsSummaryValid(uint32_t m, uint32_t largest, uint32_t karras_pairs, uint32_t max_leaf);

}  // namespace rebuild
}  // namespace srt
