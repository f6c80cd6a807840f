// scene_image.hpp -- what srt_upload_scene sends to the device, built on the host: the choices a scene's
// size makes (ChooseScenePolicy) and the device arrays with the scalars the context keeps beside them
// (BuildSceneImage).  No device: HIP's vector types only, as context.hpp; tests/cpp/test_scene_image.cpp
// links scene_image.cpp and scene_layout.cpp alone.
#pragma once

#include <hip/hip_vector_types.h>

#include <cstdint>
#include <utility>
#include <vector>

#include "launch_plan.hpp"
#include "srt_internal.hpp"

namespace srt {

// The caller's arrays (srt_upload_scene's arguments).
struct SceneArrays {
  const srt_bvh_record* bvhs;
  uint32_t n_bvhs;
  const srt_bvh_node* nodes;
  uint32_t n_nodes;
  const srt_material_obj* mats;
  const float* tex_albedo;
  uint32_t n_mats;
  const srt_triangle* tris;
  uint32_t n_tris;
  const srt_vertex* verts;
  uint32_t n_verts;
};

// The choices made from the scene's size (nodes + triangles in MB) and the environment.
struct ScenePolicy {
  bool layout;        // LayoutNodes' order (SRT_NODE_LAYOUT=0: the input order)
  bool align;         // right-child chains start on a 128-B line
  bool fused;         // global-scene mode's fused sub-steps (else the IL pattern)
  int global_waves;   // the fused instance's waves per SIMD
  bool tri_align;     // triangle slots (LayoutTris)
  int top_depth;      // the deepest top region to try (0: none)
  bool top_forced;    // SRT_TOP_DEPTH: that depth whatever the budget
  int treelet_depth;  // depth of the treelet roots
  bool tl_scene;      // treelets chosen by the scene
  bool treelets;      // the treelet copy is wanted
};
// `treelet_depth` (0: by scene size) and `treelets` (1/0 forces, -1: by scene) are the context's settings.
ScenePolicy ChooseScenePolicy(uint32_t n_nodes, uint32_t n_tris, int treelet_depth, int treelets);

// Cooperative loads (SRT_COOP builds) carry a request's float4 index in `idx_bits` bits: whether arrays of
// `n_nodes_dev` node records (slots + pad) and `n_tri_slots` triangle records fit.
constexpr bool CoopIndexFits(uint64_t n_nodes_dev, uint64_t n_tri_slots, const BuildConsts& k) {
  return 2ull * (n_nodes_dev + 1) + 8 < (1ull << k.coop_idx_bits) && 3ull * (n_tri_slots + k.tri_pad) < (1ull << k.coop_idx_bits);
}

struct SceneImage {
  // device arrays
  std::vector<float4> nodes;      // 2 per slot behind a 32-B pad, node_pad zero records past the end
  std::vector<float4> nodes_t;    // the copy with treelet roots flagged (empty: none)
  std::vector<uint32_t> troot;    // per treelet: its root's child index
  std::vector<float4> mats;       // 2 per material, one zero record appended
  std::vector<float4> tris;       // 3 per slot, tri_pad zero records past the end
  std::vector<float4> tri_uv;     // 2 per slot (empty unless a material samples a texture)
  // host records in the device layout
  std::vector<srt_bvh_record> bvhs;                      // roots remapped
  std::vector<std::pair<uint32_t, uint32_t>> bvh_tris;  // triangle slot range of each record's tree
  // scalars
  uint32_t n_slots, n_tslots, n_top, ref_or;
  int top_depth, depth;
  bool lds_ok, pairs_aligned, sampled, fused;
};

// `depth`, `tri_ranges` and `reach` are ValidateNodes' results for `in`; `lights_at_upload` the light records
// set so far (the top region's budget, launch_plan.hpp TopRegionBudget).
void BuildSceneImage(const SceneArrays& in, int depth, std::vector<std::pair<uint32_t, uint32_t>> tri_ranges,
                     const std::vector<uint8_t>& reach, const ScenePolicy& policy, const BuildConsts& k,
                     size_t lights_at_upload, SceneImage* out);

}  // namespace srt
