// The C++ mirror of include/srt_rebuild_leaf.h (include/srt/query.hpp) compiles against the C ABI, and its host half
// runs: the AssetUtils::BuildLBVH overload with max_leaf over three triangles, and its exceptions.  No device.
#include <cstdio>
#include <cstring>

#include "srt/query.hpp"
#include "srt/srt.hpp"

int main() {
  // three small triangles along x, given in the order right, left, middle
  srt_triangle t[3] = {{0, 1, 2, 7}, {3, 4, 5, 8}, {6, 7, 8, 9}};
  srt_vertex v[9]{};
  const float x0[3] = {8.0f, 0.0f, 4.0f};
  for (int k = 0; k < 3; ++k) {
    v[3 * k].vertex[0] = x0[k];
    v[3 * k + 1].vertex[0] = x0[k] + 1.0f;
    v[3 * k + 2].vertex[0] = x0[k];
    v[3 * k + 2].vertex[1] = 1.0f;
  }
  srt_bvh_node one[5]{}, n2[5]{}, n3[5]{};
  srt_triangle to1[3]{}, to[3]{};
  uint32_t order1[3] = {9, 9, 9}, order[3] = {9, 9, 9};
  srt::AssetUtils::BuildLBVH(t, 3, v, 9, one, to1, order1);
  if (order1[0] != 1 || order1[1] != 2 || order1[2] != 0) return 1;
  // max_leaf 1 through the overload: srt_bvh_build_lbvh's bytes
  srt_bvh_node again[5]{};
  if (srt::AssetUtils::BuildLBVH(t, 3, v, 9, 1u, again, to, order) != 5) return 2;
  if (std::memcmp(again, one, sizeof one) || std::memcmp(to, to1, sizeof to) || std::memcmp(order, order1, sizeof order)) return 3;
  // max_leaf 2: one pair, a leaf of one triangle and a leaf of two
  if (srt::AssetUtils::BuildLBVH(t, 3, v, 9, 2u, n2, to, order) != 3) return 4;
  if (n2[0].prim_count != 0 || n2[0].first_child_or_prim_index != 1 || n2[1].prim_count + n2[2].prim_count != 3) return 5;
  if (n2[1].first_child_or_prim_index != 0 || n2[2].first_child_or_prim_index != n2[1].prim_count) return 6;
  if (std::memcmp(order, order1, sizeof order) || n2[0].min_bounds[0] != 0.0f || n2[0].max_bounds[0] != 9.0f) return 7;
  // max_leaf 4: a leaf root
  if (srt::AssetUtils::BuildLBVH(t, 3, v, 9, 4u, n3, to, order) != 1) return 8;
  if (n3[0].prim_count != 3 || n3[0].first_child_or_prim_index != 0 || n3[0].max_bounds[0] != 9.0f) return 9;
  for (uint32_t bad : {0u, 256u}) {
    try {
      srt::AssetUtils::BuildLBVH(t, 3, v, 9, bad, n3, to, order);
      return 10;
    } catch (const std::runtime_error&) {
    }
  }
  void (srt::Query::*set_leaf)(uint32_t) = &srt::Query::SetRebuildLeaf;  // (needs a device to call)
  (void)set_leaf;
  if (srt_rebuild_leaf_abi_version() != SRT_REBUILD_LEAF_ABI_VERSION || srt_rebuild_abi_version() != 1) return 11;
  std::printf("rebuild leaf mirror OK\n");
  return 0;
}
