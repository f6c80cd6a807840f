// refit_host.cpp -- see refit_host.hpp.
#include "refit_host.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <utility>

namespace srt {
namespace refit {

namespace {

uint32_t AsUint(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  return u;
}

int Fail(std::string* err, const char* msg) {
  if (err) *err = msg;
  return SRT_ERR_INVALID;
}

}  // namespace

void LeafBox(const srt_triangle* tris, uint32_t first, uint32_t count, const srt_vertex* verts, uint32_t n_verts,
             float lo[3], float hi[3]) {
  auto vert = [&](uint32_t i, int k) -> float { return i < n_verts ? verts[i].vertex[k] : 0.0f; };
  for (int k = 0; k < 3; ++k) lo[k] = hi[k] = vert(tris[first].v0_idx, k);
  for (uint32_t t = 0; t < count; ++t) {
    const srt_triangle& tr = tris[(size_t)first + t];
    const uint32_t idx[3] = {tr.v0_idx, tr.v1_idx, tr.v2_idx};
    for (uint32_t i : idx)
      for (int k = 0; k < 3; ++k) {
        const float v = vert(i, k);
        lo[k] = FoldMin(lo[k], v);
        hi[k] = FoldMax(hi[k], v);
      }
  }
}

int RefitNodes(const srt_bvh_record* bvhs, uint32_t n_bvhs, srt_bvh_node* nodes, uint32_t n_nodes,
               const srt_triangle* tris, uint32_t n_tris, const srt_vertex* verts, uint32_t n_verts, std::string* err) {
  if ((n_bvhs && !bvhs) || (n_nodes && !nodes) || (n_tris && !tris) || (n_verts && !verts))
    return Fail(err, "null argument");
  if (n_nodes == 0 || n_bvhs == 0) return Fail(err, "scene needs at least one BVH and one node");
  // pass 1: query::BuildLayout's validation, one traversal per root
  std::vector<uint8_t> seen(n_nodes, 0);
  std::vector<uint32_t> st;
  for (uint32_t b = 0; b <= n_bvhs; ++b) {  // b == n_bvhs: node 0's tree (the ghost records)
    const uint32_t root = b < n_bvhs ? bvhs[b].first_index : 0u;
    if (root >= n_nodes) return Fail(err, "BVH first_index out of range");
    st.assign(1, root);
    while (!st.empty()) {
      const uint32_t i = st.back();
      st.pop_back();
      const srt_bvh_node& n = nodes[i];
      if (n.prim_count > 0) {
        if ((uint64_t)n.first_child_or_prim_index + n.prim_count > n_tris || n.prim_count >= 0x80000000u)
          return Fail(err, "BVH leaf references triangles out of range");
      } else {
        const uint32_t c = n.first_child_or_prim_index;
        if ((uint64_t)c + 1 >= n_nodes || seen[i])
          return Fail(err, "BVH internal node references children out of range (or a cycle)");
        seen[i] = 1;
        st.push_back(c);
        st.push_back(c + 1);
      }
    }
    std::fill(seen.begin(), seen.end(), 0);
  }
  for (uint32_t i = 0; i < n_verts; ++i)
    for (int k = 0; k < 3; ++k)
      if (!std::isfinite(verts[i].vertex[k])) return Fail(err, "srt_bvh_refit: a vertex position is not finite");
  // pass 2: post-order; a node two traversals share is refit once (its box depends on the vertices alone)
  enum : uint8_t { kNew = 0, kOpen = 1, kDone = 2 };
  std::vector<uint8_t>& state = seen;  // all zeros again
  for (uint32_t b = 0; b <= n_bvhs; ++b) {
    st.assign(1, b < n_bvhs ? bvhs[b].first_index : 0u);
    while (!st.empty()) {
      const uint32_t i = st.back();
      srt_bvh_node& n = nodes[i];
      if (state[i] == kDone) {
        st.pop_back();
      } else if (n.prim_count > 0) {
        LeafBox(tris, n.first_child_or_prim_index, n.prim_count, verts, n_verts, n.min_bounds, n.max_bounds);
        state[i] = kDone;
        st.pop_back();
      } else if (state[i] == kNew) {
        state[i] = kOpen;
        st.push_back(n.first_child_or_prim_index);
        st.push_back(n.first_child_or_prim_index + 1);
      } else {
        const srt_bvh_node& c0 = nodes[n.first_child_or_prim_index];
        const srt_bvh_node& c1 = nodes[n.first_child_or_prim_index + 1];
        for (int k = 0; k < 3; ++k) {
          n.min_bounds[k] = FoldMin(c0.min_bounds[k], c1.min_bounds[k]);
          n.max_bounds[k] = FoldMax(c0.max_bounds[k], c1.max_bounds[k]);
        }
        state[i] = kDone;
        st.pop_back();
      }
    }
  }
  return SRT_OK;
}

Schedule BuildSchedule(const query::Layout& l) {
  Schedule s;
  const uint32_t n = l.n_pairs;
  // the internal slots of pair p: the pairs it waits for
  auto child = [&](uint32_t p, int slot, uint32_t* q) {
    if (AsUint(l.pairs[4 * (size_t)p + 2 * slot + 1].w) != 0) return false;  // cnt > 0: a leaf
    *q = AsUint(l.pairs[4 * (size_t)p + 2 * slot].w);
    return true;
  };
  constexpr uint32_t kUnknown = kNoHeight;
  std::vector<uint32_t> height(n, kUnknown);
  std::vector<uint32_t> st;
  for (uint32_t p0 = 0; p0 < n; ++p0) {
    if (height[p0] != kUnknown) continue;
    st.assign(1, p0);
    while (!st.empty()) {  // (no recursion: a chain may be 2^20 levels deep)
      const uint32_t p = st.back();
      uint32_t h = 0;
      bool ready = true;
      for (int slot = 0; slot < 2; ++slot) {
        uint32_t q;
        if (!child(p, slot, &q)) continue;
        if (height[q] == kUnknown) {
          st.push_back(q);
          ready = false;
        } else {
          h = std::max(h, height[q] + 1);
        }
      }
      if (ready) {
        height[p] = h;
        st.pop_back();
      }
    }
  }
  SortByHeight(height, true, [](uint32_t p) { return p; }, &s, &s.order);  // (every pair has a height by now)
  return s;
}

}  // namespace refit
}  // namespace srt
