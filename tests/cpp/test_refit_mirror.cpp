// The C++ mirror of include/srt_refit.h (include/srt/query.hpp) compiles against the C ABI, and its host half runs:
// AssetUtils::RefitBVH over one leaf, and its exception on a scene without a BVH record.  No device.
#include <cstdio>

#include "srt/query.hpp"
#include "srt/srt.hpp"

int main() {
  srt_bvh_record b{};
  srt_bvh_node n{};
  n.prim_count = 1;
  srt_triangle t{0, 1, 2, 0};
  srt_vertex v[3]{};
  v[1].vertex[0] = 2.0f;
  v[2].vertex[1] = 3.0f;
  srt::AssetUtils::RefitBVH(&b, 1, &n, 1, &t, 1, v, 3);
  if (n.min_bounds[0] != 0.0f || n.max_bounds[0] != 2.0f || n.max_bounds[1] != 3.0f) return 1;
  try {
    srt::AssetUtils::RefitBVH(&b, 0, &n, 1, &t, 1, v, 3);
    return 2;
  } catch (const std::runtime_error&) {
  }
  void (srt::Query::*refit)(const srt_vertex*, uint32_t) = &srt::Query::Refit;  // (needs a device to call)
  (void)refit;
  std::printf("refit mirror OK\n");
  return 0;
}
