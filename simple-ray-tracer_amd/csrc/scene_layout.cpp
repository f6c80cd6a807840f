// scene_layout.cpp -- see scene_layout.hpp.
#include "scene_layout.hpp"

#include <algorithm>
#include <unordered_map>

namespace srt {

// Depth of each BVH (root depth 0) and index validation.
// Every node some traversal can reach is checked: the trees of the BVH records and node 0's (the
// ghost records past n_bvhs traverse from node 0, raytrace_compute.glsl:144-147).  `reach` marks
// them; the layouts and the upload touch no other node, so an unreachable record may hold anything.
int ValidateNodes(const srt_bvh_node* nodes, uint32_t n_nodes, uint32_t n_tris, const srt_bvh_record* bvhs,
                  uint32_t n_bvhs, int* max_depth, std::vector<std::pair<uint32_t, uint32_t>>* tri_ranges,
                  std::vector<uint8_t>* reach) {
  *max_depth = 0;
  tri_ranges->assign(n_bvhs, {0u, 0u});
  reach->assign(n_nodes, 0);
  std::vector<std::pair<uint32_t, int>> st;
  std::vector<uint8_t> seen(n_nodes, 0);
  for (uint32_t b = 0; b <= n_bvhs; ++b) {  // b == n_bvhs: node 0's tree
    uint32_t lo = 0xFFFFFFFFu, hi = 0;
    const uint32_t root = b < n_bvhs ? bvhs[b].first_index : 0u;
    if (root >= n_nodes) {
      srt::SetError("BVH first_index out of range");
      return SRT_ERR_INVALID;
    }
    st.push_back({root, 0});
    while (!st.empty()) {
      auto [i, d] = st.back();
      st.pop_back();
      (*reach)[i] = 1;
      *max_depth = std::max(*max_depth, d);
      const srt_bvh_node& n = nodes[i];
      if (n.prim_count > 0) {
        if ((uint64_t)n.first_child_or_prim_index + n.prim_count > n_tris || n.prim_count >= 0x80000000u) {
          srt::SetError("BVH leaf references triangles out of range");
          return SRT_ERR_INVALID;
        }
        lo = std::min(lo, n.first_child_or_prim_index);
        hi = std::max(hi, n.first_child_or_prim_index + n.prim_count);
      } else {
        if ((uint64_t)n.first_child_or_prim_index + 1 >= n_nodes || seen[i]) {
          srt::SetError("BVH internal node references children out of range (or a cycle)");
          return SRT_ERR_INVALID;
        }
        seen[i] = 1;
        st.push_back({n.first_child_or_prim_index, d + 1});
        st.push_back({n.first_child_or_prim_index + 1, d + 1});
      }
    }
    std::fill(seen.begin(), seen.end(), 0);
    if (b < n_bvhs) (*tri_ranges)[b] = lo < hi ? std::make_pair(lo, hi) : std::make_pair(0u, 0u);
  }
  return SRT_OK;
}

// Device node layout.  An internal step reads the current node's child pair
// and, speculatively, the pair after it (traversal.hpp, trav_internal): when
// the right child -- the one the traversal visits first -- is internal and its
// own child pair is that next pair, the step expands it too, so a descent along
// right children takes one memory round trip per two levels.  The device array
// therefore holds the pairs in the traversal's order (pre-order, right child
// first), where a right child's pair directly follows its parent's.  Only
// addresses change: every record keeps its bounds, leaf triangle range and
// count; an internal node's child index and each BVH's root are remapped.  Slot
// 0 keeps node 0 (the ghost zero records traverse from it); other roots take a
// pair's first slot with a zero record beside it.  Returns false (the identity
// layout is used) for inputs whose sibling pairs overlap, which no
// reference-built tree has.  A child pair reached from two BVH records' trees
// keeps its first placement; srt_upload_scene sets a node's "right child's
// pair follows" flag only where the remapped slots confirm it.
// `top_depth` > 0 (global-scene scenes, SRT_TOP_DEPTH): the pairs of every node at depth < top_depth are
// laid out first, in the same order, so they form the array's first `*n_top_slots` slots -- the region the
// fused instance copies into each block's LDS (traversal.hpp trav_fused) -- and the rest follows.  A pair
// on the region's last level keeps no right-spine flag (its right child's pair lies past the region).
bool LayoutNodes(const srt_bvh_node* nodes, uint32_t n_nodes, const srt_bvh_record* bvhs, uint32_t n_bvhs,
                 bool align, std::vector<uint32_t>* remap, uint32_t* n_slots, int top_depth,
                 uint32_t* n_top_slots) {
  constexpr uint32_t kUnset = 0xFFFFFFFFu;
  remap->assign(n_nodes, kUnset);
  auto& m = *remap;
  m[0] = 0;
  uint32_t next = 1;  // pairs start at odd slots (64-B aligned behind the 32-B pad)
  std::vector<uint32_t> roots{0};
  for (uint32_t b = 0; b < n_bvhs; ++b) {
    const uint32_t r = bvhs[b].first_index;
    if (m[r] == kUnset) {
      m[r] = next;
      next += 2;
    }
    roots.push_back(r);
  }
  // `align`: a chain of right-child pairs starts on a 128-B line (slot = 3 mod
  // 4: a zero pair pads before it when needed), so a step that reads a pair and
  // its right child's pair touches one line (see srt_upload_scene for when).
  uint32_t chain_next = kUnset;  // the node whose pair continues the current chain
  std::vector<uint8_t> top(top_depth > 0 ? n_nodes : 0, 0);  // nodes whose pair the first pass laid out
  std::vector<std::pair<uint32_t, int>> st;                    // (node, depth)
  for (int pass = top_depth > 0 ? 0 : 1; pass < 2; ++pass) {
    chain_next = kUnset;
    for (uint32_t r : roots) {
      st.push_back({r, 0});
      while (!st.empty()) {
        const uint32_t i = st.back().first;
        const int d = st.back().second;
        st.pop_back();
        const srt_bvh_node& n = nodes[i];
        if (n.prim_count > 0) continue;
        const uint32_t c0 = n.first_child_or_prim_index, c1 = c0 + 1;
        if (pass == 1 && !top.empty() && top[i]) {  // laid out by the first pass: descend only
          st.push_back({c0, d + 1});
          st.push_back({c1, d + 1});
          continue;
        }
        if (pass == 0 && d >= top_depth) continue;
        if (m[c0] == kUnset && m[c1] == kUnset) {
          if (align && i != chain_next && nodes[c1].prim_count == 0 && (next & 3u) != 3u) next += 2;
          m[c0] = next;
          m[c1] = next + 1;
          next += 2;
          if (pass == 0) top[i] = 1;
          chain_next = nodes[c1].prim_count == 0 ? c1 : kUnset;
          st.push_back({c0, d + 1});  // popped after c1's subtree: c1 is visited first
          st.push_back({c1, d + 1});
        } else if (m[c0] == kUnset || m[c1] != m[c0] + 1) {
          return false;  // a shared or overlapping pair
        }
      }
    }
    if (pass == 0 && n_top_slots) *n_top_slots = next;
  }
  if (top_depth <= 0 && n_top_slots) *n_top_slots = 0;
  *n_slots = next;
  return true;
}

// The slots LayoutNodes(..., top_depth) gives its top region: its first pass alone (the pairs of the nodes
// at depth < top_depth, bounded by the depth, not the tree's size); false where LayoutNodes would fail.
bool TopRegionSlots(const srt_bvh_node* nodes, uint32_t n_nodes, const srt_bvh_record* bvhs, uint32_t n_bvhs,
                    bool align, int top_depth, uint32_t* n_top) {
  std::unordered_map<uint32_t, uint32_t> m;  // the few nodes the pass places -> slot
  m[0] = 0;
  uint32_t next = 1;
  std::vector<uint32_t> roots{0};
  for (uint32_t b = 0; b < n_bvhs; ++b) {
    const uint32_t r = bvhs[b].first_index;
    if (!m.count(r)) {
      m[r] = next;
      next += 2;
    }
    roots.push_back(r);
  }
  constexpr uint32_t kUnset = 0xFFFFFFFFu;
  uint32_t chain_next = kUnset;
  std::vector<std::pair<uint32_t, int>> st;
  for (uint32_t r : roots) {
    st.push_back({r, 0});
    while (!st.empty()) {
      const uint32_t i = st.back().first;
      const int d = st.back().second;
      st.pop_back();
      const srt_bvh_node& n = nodes[i];
      if (n.prim_count > 0 || d >= top_depth) continue;
      const uint32_t c0 = n.first_child_or_prim_index, c1 = c0 + 1;
      const auto f0 = m.find(c0), f1 = m.find(c1);
      if (f0 == m.end() && f1 == m.end()) {
        if (align && i != chain_next && nodes[c1].prim_count == 0 && (next & 3u) != 3u) next += 2;
        m[c0] = next;
        m[c1] = next + 1;
        next += 2;
        chain_next = nodes[c1].prim_count == 0 ? c1 : kUnset;
        st.push_back({c0, d + 1});
        st.push_back({c1, d + 1});
      } else if (f0 == m.end() || f1 == m.end() || f1->second != f0->second + 1) {
        return false;
      }
    }
  }
  *n_top = next;
  return true;
}

// Device triangle slots for scenes read through L2 (global-scene mode).  A leaf
// of one or two triangles (the midpoint builder's leaves on a triangle soup) is
// read by one leaf step; at 48 B per record, 5 of every 8 such reads straddle
// two 128-B lines.  Here each such leaf starts at a slot whose records
// lie in one line (slot mod 8 in {0, 1, 3, 4, 6, 7} for one record, {0, 3, 6}
// for two), zero records filling the gaps; larger leaves are not padded.  The
// map is monotone, so the order is kept and a BVH's triangle range stays one
// slot range.  Returns false (identity) when two leaves' ranges partly overlap.
bool LayoutTris(const srt_bvh_node* nodes, uint32_t n_nodes, const std::vector<uint8_t>& reach, uint32_t n_tris,
                std::vector<uint32_t>* slot, uint32_t* n_slots) {
  constexpr uint32_t kUnset = 0xFFFFFFFFu;
  std::vector<uint32_t> owner(n_tris, kUnset), lead(n_tris, 0);
  for (uint32_t i = 0; i < n_nodes; ++i) {
    const srt_bvh_node& n = nodes[i];
    if (n.prim_count == 0 || !reach[i]) continue;  // (ValidateNodes range-checked the reachable leaves)
    const uint32_t f = n.first_child_or_prim_index;
    if (lead[f] != 0 && lead[f] != n.prim_count) return false;  // two leaves from one triangle, different sizes
    if (lead[f] == n.prim_count) continue;                      // the same leaf again (a shared subtree)
    for (uint32_t t = f; t < f + n.prim_count; ++t) {
      if (owner[t] != kUnset) return false;
      owner[t] = f;
    }
    lead[f] = n.prim_count;
  }
  slot->resize(n_tris);
  uint32_t s = 0;
  for (uint32_t t = 0; t < n_tris; ++t) {
    if (lead[t] == 1) {
      while ((s & 7u) == 2u || (s & 7u) == 5u) ++s;
    } else if (lead[t] == 2) {
      while ((s & 7u) % 3u != 0u) ++s;  // {0, 3, 6}
    }
    (*slot)[t] = s++;
  }
  *n_slots = s;
  return true;
}

// Kernel time of sample launches from their span records (first wave's start, last wave's end; 100 MHz
// ticks): the time during which some sample launch of the context runs, i.e. the union of the spans.
// Launches in series add their spans.  Overlapped pipeline slots dispatch a launch while its
// predecessor still runs -- it starts in the CUs the drain frees, or, when the host has enqueued several
// ahead, the hardware may run two slots' launches side by side or the later one first -- so a span then
// includes the wait for CUs another launch holds, and only the union is the launches' device time.
bool SpanRecord(const unsigned long long* ring, unsigned long long seq, unsigned long long cap, unsigned long long q,
                unsigned long long* t0, unsigned long long* t1) {
  if (q >= seq || q + cap < seq) return false;  // not written, or overwritten
  const unsigned long long* sp = ring + 2 * (q % cap);
  if (sp[1] < sp[0]) return false;
  *t0 = sp[0];
  *t1 = sp[1];
  return true;
}
// Union of the spans of records [from, to) in ms, counting only time after `after` (a tick); *last_end
// receives the latest end seen (or `after`).
double SpanUnionMs(const unsigned long long* ring, unsigned long long seq, unsigned long long cap,
                   unsigned long long from, unsigned long long to, unsigned long long after,
                   unsigned long long* last_end) {
  std::vector<std::pair<unsigned long long, unsigned long long>> iv;
  for (unsigned long long q = from; q < to; ++q) {
    unsigned long long t0, t1;
    if (SpanRecord(ring, seq, cap, q, &t0, &t1)) iv.push_back({std::max(t0, after), std::max(t1, after)});
  }
  std::sort(iv.begin(), iv.end());
  unsigned long long covered = 0, reach = after;
  for (const auto& [a, b] : iv) {
    const unsigned long long lo = std::max(a, reach);
    if (b > lo) covered += b - lo;
    reach = std::max(reach, b);
  }
  if (last_end) *last_end = reach;
  return (double)covered * 1e-5;
}

}  // namespace srt
