// query_host.cpp -- see query_host.hpp.
#include "query_host.hpp"

#include <algorithm>
#include <cstring>
#include <utility>

namespace srt {
namespace query {

namespace {

float AsFloat(uint32_t u) {
  float f;
  std::memcpy(&f, &u, 4);
  return f;
}

int Fail(std::string* err, const char* msg) {
  if (err) *err = msg;
  return SRT_ERR_INVALID;
}

}  // namespace

int BuildLayout(const srt_bvh_record* bvhs, uint32_t n_bvhs, const srt_bvh_node* nodes, uint32_t n_nodes,
                const srt_triangle* tris, uint32_t n_tris, const srt_vertex* verts, uint32_t n_verts, Layout* out,
                std::string* err) {
  if (!out || (n_bvhs && !bvhs) || (n_nodes && !nodes) || (n_tris && !tris) || (n_verts && !verts))
    return Fail(err, "null argument");
  if (n_nodes == 0 || n_bvhs == 0) return Fail(err, "scene needs at least one BVH and one node");
  *out = Layout();
  // pass 1: validation, depth, and a pair index for every child pair reached (keyed by its first child)
  std::vector<uint32_t> pair_of(n_nodes, kNoPair);
  std::vector<uint8_t> seen(n_nodes, 0);
  std::vector<std::pair<uint32_t, int>> st;
  for (uint32_t b = 0; b <= n_bvhs; ++b) {  // b == n_bvhs: node 0's tree (the ghost records)
    const uint32_t root = b < n_bvhs ? bvhs[b].first_index : 0u;
    if (root >= n_nodes) return Fail(err, "BVH first_index out of range");
    st.clear();
    st.push_back({root, 0});
    while (!st.empty()) {
      const uint32_t i = st.back().first;
      const int d = st.back().second;
      st.pop_back();
      out->depth = std::max(out->depth, d);
      const srt_bvh_node& n = nodes[i];
      if (n.prim_count > 0) {
        if ((uint64_t)n.first_child_or_prim_index + n.prim_count > n_tris || n.prim_count >= 0x80000000u)
          return Fail(err, "BVH leaf references triangles out of range");
        out->max_leaf = std::max(out->max_leaf, n.prim_count);
      } else {
        const uint32_t c = n.first_child_or_prim_index;
        if ((uint64_t)c + 1 >= n_nodes || seen[i])
          return Fail(err, "BVH internal node references children out of range (or a cycle)");
        seen[i] = 1;
        if (pair_of[c] == kNoPair) pair_of[c] = out->n_pairs++;
        st.push_back({c, d + 1});  // popped second: the traversal visits the right child first
        st.push_back({c + 1, d + 1});
      }
    }
    std::fill(seen.begin(), seen.end(), 0);
  }
  // pass 2: the records
  auto record = [&](uint32_t i, F4* lo, F4* hi) {
    const srt_bvh_node& n = nodes[i];
    const uint32_t ref = n.prim_count > 0 ? n.first_child_or_prim_index : pair_of[n.first_child_or_prim_index];
    *lo = F4{n.min_bounds[0], n.min_bounds[1], n.min_bounds[2], AsFloat(ref)};
    *hi = F4{n.max_bounds[0], n.max_bounds[1], n.max_bounds[2], AsFloat(n.prim_count)};
  };
  out->pairs.assign(4 * (size_t)std::max(out->n_pairs, 1u), F4{0, 0, 0, 0});
  for (uint32_t c = 0; c + 1 < n_nodes; ++c) {
    const uint32_t p = pair_of[c];
    if (p == kNoPair) continue;
    record(c, &out->pairs[4 * (size_t)p], &out->pairs[4 * (size_t)p + 1]);
    record(c + 1, &out->pairs[4 * (size_t)p + 2], &out->pairs[4 * (size_t)p + 3]);
  }
  out->roots.assign(2 * ((size_t)n_bvhs + 1), F4{0, 0, 0, 0});
  for (uint32_t b = 0; b <= n_bvhs; ++b)
    record(b < n_bvhs ? bvhs[b].first_index : 0u, &out->roots[2 * (size_t)b], &out->roots[2 * (size_t)b + 1]);
  // triangles: edges precomputed (the same fp32 subtractions IntersectsTriangle makes); a vertex index past
  // the array reads zeros, as an out-of-bounds SSBO read does
  out->tris.assign(3 * ((size_t)n_tris + kTriPad), F4{0, 0, 0, 0});
  auto vert = [&](uint32_t i, int k) -> float { return i < n_verts ? verts[i].vertex[k] : 0.0f; };
  for (uint32_t t = 0; t < n_tris; ++t) {
    const srt_triangle& tr = tris[t];
    float v0[3], e1[3], e2[3];
    for (int k = 0; k < 3; ++k) {
      v0[k] = vert(tr.v0_idx, k);
      e1[k] = vert(tr.v1_idx, k) - v0[k];
      e2[k] = vert(tr.v2_idx, k) - v0[k];
    }
    out->tris[3 * (size_t)t + 0] = F4{v0[0], v0[1], v0[2], e1[0]};
    out->tris[3 * (size_t)t + 1] = F4{e1[1], e1[2], e2[0], e2[1]};
    out->tris[3 * (size_t)t + 2] = F4{e2[2], AsFloat(tr.material_idx), AsFloat(t), 0.0f};
  }
  return SRT_OK;
}

StackPlan PlanStack(const Layout& l, uint32_t n_tris) {
  StackPlan p;
  p.entries = l.depth + 1;
  p.packed = l.n_pairs < (1u << 24) && n_tris < (1u << 24) && l.max_leaf < 256u;
  const size_t dwords = (size_t)kBlock * (p.packed ? 2 : 3) * (size_t)p.entries;
  p.in_hbm = (size_t)kBlock * 3 * (size_t)p.entries * sizeof(uint32_t) > kLdsStackMax;
  p.lds_bytes = p.in_hbm ? 0 : dwords * sizeof(uint32_t);
  p.hbm_block_bytes = p.in_hbm ? dwords * sizeof(uint32_t) : 0;
  return p;
}

}  // namespace query
}  // namespace srt
