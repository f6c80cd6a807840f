// The C++ mirror of include/srt_rebuild.h (include/srt/query.hpp) compiles against the C ABI, and its host half runs:
// AssetUtils::BuildLBVH over two triangles, and its exception on an empty mesh.  No device.
#include <cstdio>

#include "srt/query.hpp"
#include "srt/srt.hpp"

int main() {
  srt_triangle t[2] = {{0, 1, 2, 7}, {3, 4, 5, 9}};
  srt_vertex v[6]{};
  v[0].vertex[0] = 8.0f;  // triangle 0 lies at x in [8, 10], triangle 1 at x in [0, 2]: the order swaps them
  v[1].vertex[0] = 10.0f;
  v[2].vertex[0] = 8.0f;
  v[2].vertex[1] = 3.0f;
  v[4].vertex[0] = 2.0f;
  v[5].vertex[1] = 3.0f;
  srt_bvh_node n[3]{};
  srt_triangle to[2]{};
  uint32_t order[2] = {9, 9};
  srt::AssetUtils::BuildLBVH(t, 2, v, 6, n, to, order);
  if (order[0] != 1 || order[1] != 0 || to[0].material_idx != 9 || to[1].material_idx != 7) return 1;
  if (n[0].prim_count != 0 || n[0].first_child_or_prim_index != 1 || n[1].prim_count != 1 || n[2].prim_count != 1) return 2;
  if (n[0].min_bounds[0] != 0.0f || n[0].max_bounds[0] != 10.0f || n[1].max_bounds[0] != 2.0f || n[2].min_bounds[0] != 8.0f) return 3;
  try {
    srt::AssetUtils::BuildLBVH(t, 0, v, 6, n, to, order);
    return 4;
  } catch (const std::runtime_error&) {
  }
  void (srt::Query::*enable)() = &srt::Query::EnableRebuild;  // (both need a device to call)
  void (srt::Query::*rebuild)(const srt_vertex*, uint32_t) = &srt::Query::Rebuild;
  (void)enable;
  (void)rebuild;
  if (srt_rebuild_abi_version() != SRT_REBUILD_ABI_VERSION) return 5;
  std::printf("rebuild mirror OK\n");
  return 0;
}
