// scene_image.cpp -- see scene_image.hpp.
#include "scene_image.hpp"

#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "scene_image_maps.hpp"
#include "scene_layout.hpp"

namespace srt {

namespace {

float F32(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }
uint32_t U32(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }

}  // namespace

ScenePolicy ChooseScenePolicy(uint32_t n_nodes, uint32_t n_tris, int treelet_depth, int treelets) {
  ScenePolicy p{};
  const char* lay_env = std::getenv("SRT_NODE_LAYOUT");
  p.layout = !(lay_env && lay_env[0] == '0');
  // Line-aligned chains pay where the tree streams from HBM: fewer lines per
  // step (C5, 10 M triangles: 505 -> 578 Mrays/s; 3 M: 774 -> 823).  A scene
  // the 256-MB Infinity Cache holds runs latency-bound and is faster dense
  // (300 k: 1929 vs 1695; 1 M: 1234 vs 1088), though it then misses more
  // often in L2.  Measured crossover between 100 and 300 MB of nodes +
  // triangles; SRT_NODE_ALIGN=1/0 forces either.
  const char* al_env = std::getenv("SRT_NODE_ALIGN");
  const double scene_mb = (32.0 * n_nodes + 48.0 * n_tris) / (1 << 20);
  p.align = al_env ? al_env[0] == '1' : scene_mb >= 192.0;
  // Global-scene traversal schedule: fused sub-steps (trav_fused: one memory
  // round trip per step for both node kinds) while the kernel waits on latency
  // (1 M, 101 MB: 1232 -> 1373 Mrays/s; 262 k torus knot 4576 -> 5432; 3 M,
  // 336 MB: 832 -> 869); the IL pattern once the tree streams from HBM and
  // the bytes bound it (10 M, 1.1 GB, at 1080p: 543 vs 528).  Crossover taken
  // at 600 MB; SRT_GLOBAL_FUSED_MODE=1/0 forces either.
  const char* fu_env = std::getenv("SRT_GLOBAL_FUSED_MODE");
  p.fused = fu_env ? fu_env[0] == '1' : scene_mb < 600.0;
  // Waves per SIMD of the fused instance: 5 (8-entry rings, some spills) while the tree is small
  // enough that the extra rays in flight pay (torus knot 262 k, 20 MB: 5,405 -> 5,650 Mrays/s; Rubik
  // forced global +6%; 100 k +2%; 300 k, 30 MB: +1%), else 4 (1 M, 101 MB: -7% with 5; 3 M: -7%).
  // Crossover taken at 48 MB; SRT_GLOBAL_WAVES_MODE=4/5 forces either.
  const char* gw_env = std::getenv("SRT_GLOBAL_WAVES_MODE");
  p.global_waves = gw_env ? (gw_env[0] == '5' ? 5 : 4) : (scene_mb < 48.0 ? 5 : 4);
  // Triangle slots (LayoutTris) for every scene read through L2 (none of 1 MB fits the LDS copy):
  // fewer lines per leaf step (A/B on one box, kernel ms: C5 10 M 4096² 820 -> 773 with the IL leaf
  // step's own-record reads, 3 M 58.4 -> 56.5, 1 M 34.1 -> 32.6, torus knot 27.4 -> 27.4, Rubik
  // unchanged).  SRT_TRI_ALIGN=1/0 forces either.  Leaves and each BVH's triangle range are
  // remapped; a record keeps its triangle's input index (C.z) for the closest-hit query.
  const char* ta_env = std::getenv("SRT_TRI_ALIGN");
  p.tri_align = ta_env ? ta_env[0] == '1' : scene_mb >= 1.0;
  // The fused instance's LDS copy of the tree's top levels (traversal.hpp trav_fused): LDS reads bypass
  // the vector-memory pipeline that bounds these kernels.  As deep as fits the
  // budget, from 12 levels down (BuildSceneImage); SRT_TOP_DEPTH=d forces d levels, 0 none.
  const char* td_env = std::getenv("SRT_TOP_DEPTH");
  p.top_forced = td_env != nullptr;
  if (p.fused && scene_mb >= 1.0 && !(td_env && std::atoi(td_env) <= 0)) p.top_depth = td_env ? std::atoi(td_env) : 12;
  // Treelet scheduling (wavefront mode): chosen for trees past the Infinity Cache, with ~1 MB of nodes +
  // triangles per treelet (SRT_TREELETS=1/0 forces it, SRT_TREELET_DEPTH sets the depth)
  p.treelet_depth = treelet_depth;
  if (p.treelet_depth == 0) {
    p.treelet_depth = 1;
    while (p.treelet_depth < kTopStack - 1 && scene_mb / (double)(1u << (p.treelet_depth + 1)) >= 1.0) ++p.treelet_depth;
  }
  p.tl_scene = false;  // opt-in (measured slower than sample_kernel: DESIGN.md section 5, "Wavefront mode")
  p.treelets = treelets >= 0 ? treelets == 1 : p.tl_scene;
  return p;
}

void BuildSceneImage(const SceneArrays& in, int depth, std::vector<std::pair<uint32_t, uint32_t>> tri_ranges,
                     const std::vector<uint8_t>& reach, const ScenePolicy& policy, const BuildConsts& k,
                     size_t lights_at_upload, SceneImage* out) {
  BuildSceneImageMaps(in, depth, std::move(tri_ranges), reach, policy, k, lights_at_upload, out, nullptr);
}

void BuildSceneImageMaps(const SceneArrays& in, int depth, std::vector<std::pair<uint32_t, uint32_t>> tri_ranges,
                         const std::vector<uint8_t>& reach, const ScenePolicy& policy, const BuildConsts& k,
                         size_t lights_at_upload, SceneImage* out, SceneMaps* maps) {
  const srt_bvh_node* nodes = in.nodes;
  const uint32_t n_nodes = in.n_nodes, n_tris = in.n_tris, n_mats = in.n_mats, n_verts = in.n_verts;
  SceneImage& img = *out;
  img = SceneImage{};
  img.depth = depth;
  // triangle slots; the slots stay below 3 n_tris: a gap is at most two records per leaf
  std::vector<uint32_t> tslot;
  uint32_t n_tslots = n_tris;
  const bool tris_laid =
      policy.tri_align && n_tris < (1u << 30) && LayoutTris(nodes, n_nodes, reach, n_tris, &tslot, &n_tslots);
  auto tsl = [&](uint32_t t) { return tris_laid ? tslot[t] : t; };
  uint32_t max_leaf = 0;
  for (uint32_t i = 0; i < n_nodes; ++i)
    if (reach[i]) max_leaf = std::max(max_leaf, nodes[i].prim_count);
  // The top region: laid out first, as deep as fits the budget.  The ring's entry size is the one the
  // launch will use (lds_ok below, here with the dense node count: a line-aligned layout's padding only
  // matters past 2^24 slots, where the launch then finds the region too large and skips it).  A depth's
  // region size comes from the layout's first pass alone (TopRegionSlots, bounded by the depth); the full
  // layout runs once.
  uint32_t n_top = 0;
  int top_depth = policy.top_depth;
  if (top_depth > 0) {
    const size_t budget =
        TopRegionBudget(k, policy.global_waves, PackedEntries(n_tslots, n_nodes, max_leaf, k), lights_at_upload);
    for (; top_depth > 0; --top_depth) {  // the deepest whole levels that fit
      if (!TopRegionSlots(nodes, n_nodes, in.bvhs, in.n_bvhs, policy.align, top_depth, &n_top)) {
        top_depth = 0;
        break;
      }
      if (policy.top_forced || TopRegionBytes(k, 2 * (size_t)n_top + 2) <= budget) break;
    }
  }
  // nodes: 32-B records behind a 32-B pad so sibling pairs are 64-B aligned, in the traversal's order
  // (LayoutNodes; unreachable nodes are dropped), and zero pairs past the end for the internal step's
  // speculative read
  std::vector<uint32_t> remap;
  uint32_t n_slots = n_nodes;
  const bool laid = policy.layout &&
                    LayoutNodes(nodes, n_nodes, in.bvhs, in.n_bvhs, policy.align, &remap, &n_slots, top_depth, &n_top);
  if (!laid) {
    n_top = 0;
    remap.resize(n_nodes);
    for (uint32_t i = 0; i < n_nodes; ++i) remap[i] = i;
    n_slots = n_nodes;
  }
  for (auto& r : tri_ranges)
    if (r.first < r.second) r = {tsl(r.first), tsl(r.second - 1) + 1};
  img.nodes.assign(2 * ((size_t)n_slots + 1 + k.node_pad), make_float4(0, 0, 0, 0));
  std::vector<float4>& hn = img.nodes;
  bool pairs_aligned = true;
  for (uint32_t i = 0; i < n_nodes; ++i) {
    // (a node no traversal reaches keeps a zero record: its indices were never range-checked)
    if (remap[i] == 0xFFFFFFFFu || !reach[i]) continue;
    const srt_bvh_node& n = nodes[i];
    uint32_t first = n.first_child_or_prim_index;
    if (n.prim_count == 0) {  // internal: c0's slot, less 1 when c1 is internal (its pair then follows)
      // The flag promises that c1's own child pair is the next pair of the array.  LayoutNodes
      // places it there whenever it lays the pair out itself; a pair shared with an earlier
      // BVH record's tree keeps its first placement, so the flag is set only when the
      // remapped slots say so.
      const uint32_t c0 = n.first_child_or_prim_index;
      const srt_bvh_node& n1 = nodes[c0 + 1];
      first = remap[first];
      if (laid && n1.prim_count == 0 && remap[n1.first_child_or_prim_index] == remap[c0] + 2) first -= 1;
      if (((first | (laid ? 1u : 0u)) & 1u) == 0) pairs_aligned = false;  // overlapping sibling pairs
    } else {
      first = tsl(first);
    }
    hn[2 * (size_t)remap[i] + 2] = make_float4(n.min_bounds[0], n.min_bounds[1], n.min_bounds[2], F32(first));
    hn[2 * (size_t)remap[i] + 3] = make_float4(n.max_bounds[0], n.max_bounds[1], n.max_bounds[2], F32(n.prim_count));
  }
  // Treelet scheduling (wavefront mode, wavefront.hpp): a copy of the node array in which every internal
  // node at depth td of some tree (walked from every BVH root and from slot 0, where the ghost records
  // start) is a treelet root -- its count treelet_cnt, its child index the treelet's id -- and whose
  // nodes with a treelet root as right child lose the right-spine flag (the top kernel must make the root
  // current, not expand it).  Every path deeper than td passes a root, so the top-level stack holds < td
  // entries.
  const int td = policy.treelet_depth;
  if (policy.treelets && max_leaf < k.treelet_cnt && depth > td) {
    std::vector<float4> hf(hn);
    std::vector<uint32_t> troot;
    std::vector<int32_t> tid_of(n_slots, -1);
    std::vector<uint32_t> roots{0};
    for (uint32_t b = 0; b < in.n_bvhs; ++b) roots.push_back(remap[in.bvhs[b].first_index]);
    std::vector<std::pair<uint32_t, int>> st;
    const uint32_t ror = laid ? 1u : 0u;
    for (uint32_t r : roots) {
      st.push_back({r, 0});
      while (!st.empty()) {
        auto [sl, d] = st.back();
        st.pop_back();
        if (U32(hn[2 * (size_t)sl + 3].w) != 0u || tid_of[sl] >= 0) continue;  // a leaf, or a root already
        const uint32_t first = U32(hn[2 * (size_t)sl + 2].w);
        if (d == td) {
          tid_of[sl] = (int32_t)troot.size();
          troot.push_back(first);
          hf[2 * (size_t)sl + 2].w = F32((uint32_t)tid_of[sl]);
          hf[2 * (size_t)sl + 3].w = F32(k.treelet_cnt);
          continue;
        }
        const uint32_t ref0 = first | ror;
        st.push_back({ref0, d + 1});
        st.push_back({ref0 + 1, d + 1});
      }
    }
    for (uint32_t sl = 0; sl < n_slots && ror; ++sl) {  // no right-spine step onto a treelet root
      const uint32_t first = U32(hn[2 * (size_t)sl + 2].w);
      if (tid_of[sl] >= 0 || U32(hn[2 * (size_t)sl + 3].w) != 0u || (first & 1u)) continue;
      if (first + 2 < n_slots && tid_of[first + 2] >= 0) hf[2 * (size_t)sl + 2].w = F32(first | 1u);
    }
    if (!troot.empty()) {
      img.nodes_t = std::move(hf);
      img.troot = std::move(troot);
    }
  }
  // materials -> shading materials (raytrace_utils.glsl:140-175); one zero
  // record appended for out-of-range material indices (OOB SSBO reads = 0)
  img.mats.assign(2 * ((size_t)n_mats + 1), make_float4(0, 0, 0, 0));
  bool sampled = false;
  for (uint32_t i = 0; i <= n_mats; ++i) {
    srt_material_obj m{};
    if (i < n_mats) m = in.mats[i];
    float alb[3] = {m.diffuse[0], m.diffuse[1], m.diffuse[2]};
    uint32_t tex = 0;  // sampled texture + 1 (0: constant albedo)
    if (m.use_texture) {
      for (int c = 0; c < 3; ++c) alb[c] = in.tex_albedo ? in.tex_albedo[3 * (size_t)i + c] : 0.0f;
      if (!in.tex_albedo) {
        const uint64_t h = (uint64_t)m.handle[0] | ((uint64_t)m.handle[1] << 32);
        tex = h < 0xFFFFFFFFull ? (uint32_t)h + 1 : 0xFFFFFFFFu;  // unknown handles sample zero
        sampled = true;
      }
    }
    const float rough = 1.0f / (m.specular_ex + 0.0000001f);
    img.mats[2 * (size_t)i] = make_float4(alb[0], alb[1], alb[2], rough);
    img.mats[2 * (size_t)i + 1] = make_float4(m.specular[0], m.specular[1], m.specular[2], F32(tex));
  }
  // triangles (at their slots): v0, e1 = v1 - v0, e2 = v2 - v0, material, input index
  // tri_pad zero records past the end: a multi-triangle leaf step may read (and discard) them
  img.tris.assign(3 * ((size_t)n_tslots + k.tri_pad), make_float4(0, 0, 0, 0));
  auto vert = [&](uint32_t i, int c) -> float { return i < n_verts ? in.verts[i].vertex[c] : 0.0f; };
  for (uint32_t t = 0; t < n_tris; ++t) {
    const size_t st = tsl(t);
    const srt_triangle& tr = in.tris[t];
    float v0[3], e1[3], e2[3];
    for (int c = 0; c < 3; ++c) {
      v0[c] = vert(tr.v0_idx, c);
      e1[c] = vert(tr.v1_idx, c) - v0[c];
      e2[c] = vert(tr.v2_idx, c) - v0[c];
    }
    const uint32_t mi = tr.material_idx < n_mats ? tr.material_idx : n_mats;
    img.tris[3 * st + 0] = make_float4(v0[0], v0[1], v0[2], e1[0]);
    img.tris[3 * st + 1] = make_float4(e1[1], e1[2], e2[0], e2[1]);
    img.tris[3 * st + 2] = make_float4(e2[2], F32(mi), F32(t), 0.0f);
  }
  // vertex uvs per triangle, for the materials that sample a texture
  if (sampled) {
    img.tri_uv.assign(2 * (size_t)n_tslots, make_float4(0, 0, 0, 0));
    auto uv = [&](uint32_t i, int c) -> float { return i < n_verts ? in.verts[i].texture[c] : 0.0f; };
    for (uint32_t t = 0; t < n_tris; ++t) {
      const srt_triangle& tr = in.tris[t];
      const size_t st = tsl(t);
      img.tri_uv[2 * st] = make_float4(uv(tr.v0_idx, 0), uv(tr.v0_idx, 1), uv(tr.v1_idx, 0), uv(tr.v1_idx, 1));
      img.tri_uv[2 * st + 1] = make_float4(uv(tr.v2_idx, 0), uv(tr.v2_idx, 1), 0.0f, 0.0f);
    }
  }
  img.bvhs.assign(in.bvhs, in.bvhs + in.n_bvhs);
  for (auto& r : img.bvhs) r.first_index = remap[r.first_index];  // roots in the device layout
  img.bvh_tris = std::move(tri_ranges);
  img.n_slots = n_slots;
  img.n_tslots = n_tslots;
  img.n_top = n_top;
  img.top_depth = n_top > 0 ? top_depth : 0;
  img.ref_or = laid ? 1u : 0u;
  img.sampled = sampled;
  img.pairs_aligned = pairs_aligned;
  img.lds_ok = PackedEntries(n_tslots, n_slots, max_leaf, k);
  // larger arrays than cooperative loads index (only reachable with SRT_GLOBAL_FUSED_MODE=1 past 600 MB)
  // take the IL instance
  img.fused = policy.fused && !(k.coop && !CoopIndexFits((uint64_t)n_slots + k.node_pad, n_tslots, k));
  if (maps) {
    if (!tris_laid) {
      tslot.resize(n_tris);
      for (uint32_t t = 0; t < n_tris; ++t) tslot[t] = t;
    }
    maps->node_slot = std::move(remap);
    maps->tri_slot = std::move(tslot);
  }
}

}  // namespace srt
