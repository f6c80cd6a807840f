// stage_host.hpp -- host-only helpers the stage objects share (query.hip, denoise.hip, temporal.hip, surface.hip).
// No device, no HIP header: tests/cpp/test_stage_host.cpp links stage_host.cpp with the scene producers alone.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/srt_amd.h"

namespace srt {
namespace stage {

// A size as srt_*_get_int reports it: itself, or INT_MAX when it does not fit.
int SaturateInt(size_t v);

// `alignment` is a power of two.  NULL counts as aligned: the entry points test for a missing pointer separately.
bool Aligned(const void* p, size_t alignment);

// The flattened arrays of an srt_scene (srt_scene_sizes / srt_scene_copy).
struct SceneArrays {
  std::vector<srt_bvh_record> bvhs;
  std::vector<srt_bvh_node> nodes;
  std::vector<srt_material_obj> mats;
  std::vector<float> tex_albedo;  // 3 per material
  std::vector<srt_triangle> tris;
  std::vector<srt_vertex> verts;
};
// SRT_OK, or what srt_scene_sizes / srt_scene_copy return (SRT_ERR_INVALID for a NULL scene or a NULL `out`).
int CopyScene(const srt_scene* s, SceneArrays* out);

}  // namespace stage
}  // namespace srt
