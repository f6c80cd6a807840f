// stage_host.cpp -- see stage_host.hpp.
#include "stage_host.hpp"

#include <climits>

namespace srt {
namespace stage {

int SaturateInt(size_t v) { return v < (size_t)INT_MAX ? (int)v : INT_MAX; }

bool Aligned(const void* p, size_t alignment) { return ((uintptr_t)p & (alignment - 1)) == 0; }

int CopyScene(const srt_scene* s, SceneArrays* out) {
  if (!out) return SRT_ERR_INVALID;
  uint32_t sz[5] = {0, 0, 0, 0, 0};
  if (int rc = srt_scene_sizes(s, sz)) return rc;
  out->bvhs.resize(sz[0]);
  out->nodes.resize(sz[1]);
  out->mats.resize(sz[2]);
  out->tex_albedo.resize(3 * (size_t)sz[2]);
  out->tris.resize(sz[3]);
  out->verts.resize(sz[4]);
  return srt_scene_copy(s, out->bvhs.data(), out->nodes.data(), out->mats.data(), out->tex_albedo.data(), out->tris.data(),
                        out->verts.data());
}

}  // namespace stage
}  // namespace srt
