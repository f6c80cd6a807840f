// scene_image_maps.hpp -- BuildSceneImage with the two maps it computes on the way: where each input node and
// each input triangle went in the device layout.  The scene refit (scene_refit.hip) needs them; the upload does
// not, and scene_image.hpp -- a header of pathtrace.hip, part of the code hash -- stays as it is.  Host only.
#pragma once

#include <cstdint>
#include <utility>
#include <vector>

#include "scene_image.hpp"

namespace srt {

struct SceneMaps {
  std::vector<uint32_t> node_slot;  // per input node: its slot of the device node array (0xFFFFFFFF: not placed)
  std::vector<uint32_t> tri_slot;   // per input triangle: its slot of the device triangle array
};

// BuildSceneImage's body: the same image from the same arguments; `maps` (may be null) receives the maps.
void BuildSceneImageMaps(const SceneArrays& in, int depth, std::vector<std::pair<uint32_t, uint32_t>> tri_ranges,
                         const std::vector<uint8_t>& reach, const ScenePolicy& policy, const BuildConsts& k,
                         size_t lights_at_upload, SceneImage* out, SceneMaps* maps);

}  // namespace srt
