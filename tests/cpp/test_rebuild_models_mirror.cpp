// The C++ mirror of include/srt_rebuild_models.h (include/srt/query.hpp) compiles against the C ABI, and its host half
// runs: AssetUtils::BuildLBVHModels over two records of two and one triangles, and its exceptions.  No device.
#include <cstdio>
#include <cstring>

#include "srt/query.hpp"
#include "srt/srt.hpp"

int main() {
  // record 0: triangles 0 (right) and 2 (left) under a pair at nodes 1, 2; record 1: triangle 1, a leaf root at node 3
  srt_triangle t[3] = {{0, 1, 2, 7}, {3, 4, 5, 8}, {6, 7, 8, 9}};
  srt_vertex v[9]{};
  const float x0[3] = {8.0f, 20.0f, 4.0f};
  for (int k = 0; k < 3; ++k) {
    v[3 * k].vertex[0] = x0[k];
    v[3 * k + 1].vertex[0] = x0[k] + 1.0f;
    v[3 * k + 2].vertex[0] = x0[k];
    v[3 * k + 2].vertex[1] = 1.0f;
  }
  srt_bvh_node nodes[4]{};
  nodes[0].first_child_or_prim_index = 1;
  nodes[1].first_child_or_prim_index = 0;
  nodes[1].prim_count = 1;
  nodes[2].first_child_or_prim_index = 2;
  nodes[2].prim_count = 1;
  nodes[3].first_child_or_prim_index = 1;
  nodes[3].prim_count = 1;
  srt_bvh_record bvhs[2]{};
  bvhs[0].count = 3;
  bvhs[1].first_index = 3;
  bvhs[1].count = 1;
  bvhs[1].frame[0] = 2.0f;
  srt_bvh_record bo[2]{};
  srt_bvh_node no[5]{};
  srt_triangle to[3]{};
  uint32_t order[3] = {9, 9, 9};
  if (srt::AssetUtils::BuildLBVHModels(bvhs, 2, nodes, 4, t, 3, v, 9, 1u, bo, no, to, order) != 4) return 1;
  if (order[0] != 2 || order[1] != 0 || order[2] != 1) return 2;  // record 0 by key, then record 1
  if (bo[0].first_index != 0 || bo[1].first_index != 3 || bo[1].frame[0] != 2.0f) return 3;
  if (no[0].prim_count != 0 || no[0].first_child_or_prim_index != 1 || no[0].min_bounds[0] != 4.0f || no[0].max_bounds[0] != 9.0f) return 4;
  if (no[3].prim_count != 1 || no[3].first_child_or_prim_index != 2 || no[3].min_bounds[0] != 20.0f) return 5;
  if (to[0].material_idx != 9 || to[2].material_idx != 8) return 6;
  // max_leaf 2: both records leaf roots
  if (srt::AssetUtils::BuildLBVHModels(bvhs, 2, nodes, 4, t, 3, v, 9, 2u, bo, no, to, order) != 2) return 7;
  if (no[0].prim_count != 2 || no[0].first_child_or_prim_index != 0 || no[1].prim_count != 1 || bo[1].first_index != 1) return 8;
  bvhs[1].first_index = 2;  // record 1 names a triangle of record 0, and triangle 1 has no record
  try {
    srt::AssetUtils::BuildLBVHModels(bvhs, 2, nodes, 4, t, 3, v, 9, 1u, bo, no, to, order);
    return 9;
  } catch (const std::runtime_error& e) {
    if (!std::strstr(e.what(), "exactly one BVH record")) return 10;
  }
  void (srt::Query::*enable)() = &srt::Query::EnableRebuildModels;  // (needs a device to call)
  (void)enable;
  if (srt_rebuild_models_abi_version() != SRT_REBUILD_MODELS_ABI_VERSION || srt_rebuild_leaf_abi_version() != 1 ||
      srt_rebuild_abi_version() != 1)
    return 11;
  std::printf("rebuild models mirror OK\n");
  return 0;
}
