// scene_refit_host.cpp -- see scene_refit_host.hpp.
#include "scene_refit_host.hpp"

#include <algorithm>

namespace srt {
namespace scene_refit {

bool BuildSchedule(const uint32_t* ref, const uint32_t* cnt, uint32_t n_slots, uint32_t ref_or, const uint32_t* roots,
                   uint32_t n_roots, const uint32_t* tri_of_slot, uint32_t n_tri_slots, uint32_t n_tris, Schedule* out) {
  Schedule s;
  constexpr uint32_t kUnknown = 0xFFFFFFFFu, kOpen = 0xFFFFFFFEu;
  std::vector<uint32_t> height(n_slots, kUnknown);
  std::vector<uint32_t> st;
  for (uint32_t r = 0; r < n_roots; ++r) {
    if (roots[r] >= n_slots) return false;
    st.assign(1, roots[r]);
    while (!st.empty()) {  // (no recursion: a chain may be 2^20 levels deep)
      const uint32_t i = st.back();
      if (height[i] < kOpen) {  // done, by this root or an earlier one
        st.pop_back();
      } else if (cnt[i] > 0) {
        const uint32_t t = tri_of_slot ? (ref[i] < n_tri_slots ? tri_of_slot[ref[i]] : kUnknown) : ref[i];
        if (ref[i] >= n_tri_slots || t >= n_tris || cnt[i] > n_tris - t) return false;
        height[i] = 0;
        st.pop_back();
      } else {
        const uint32_t c0 = ref[i] | ref_or;
        if ((uint64_t)c0 + 1 >= n_slots) return false;
        if (height[i] == kUnknown) {
          height[i] = kOpen;
          st.push_back(c0);
          st.push_back(c0 + 1);
        } else {  // open, and both children are done -- unless one of them is this node's ancestor
          if (height[c0] >= kOpen || height[c0 + 1] >= kOpen) return false;
          height[i] = 1 + std::max(height[c0], height[c0 + 1]);
          st.pop_back();
        }
      }
    }
  }
  for (uint32_t i = 0; i < n_slots; ++i)
    if (height[i] != kUnknown) s.heights = std::max(s.heights, height[i] + 1);
  s.first.assign((size_t)s.heights + 1, 0);
  for (uint32_t i = 0; i < n_slots; ++i)
    if (height[i] != kUnknown) ++s.first[(size_t)height[i] + 1];
  for (uint32_t h = 0; h < s.heights; ++h) s.first[h + 1] += s.first[h];
  s.order.resize(s.first[s.heights]);
  std::vector<uint32_t> at(s.first.begin(), s.first.end() - 1);
  for (uint32_t i = 0; i < n_slots; ++i) {
    if (height[i] == kUnknown) continue;
    const uint32_t t = cnt[i] > 0 ? (tri_of_slot ? tri_of_slot[ref[i]] : ref[i]) : 0u;
    s.order[at[height[i]]++] = Entry{i, t};
  }
  s.tail_begin = s.heights;
  while (s.tail_begin > 0 && s.first[s.tail_begin] - s.first[s.tail_begin - 1] <= kBlock) --s.tail_begin;
  s.launches = (n_tris > 0 ? 1u : 0u) + s.tail_begin + 1;
  *out = std::move(s);
  return true;
}

std::vector<uint32_t> BuildTriples(const srt_triangle* tris, uint32_t n_tris, const uint32_t* tri_slot) {
  std::vector<uint32_t> t(4 * (size_t)n_tris);
  for (uint32_t i = 0; i < n_tris; ++i) {
    t[4 * (size_t)i + 0] = tris[i].v0_idx;
    t[4 * (size_t)i + 1] = tris[i].v1_idx;
    t[4 * (size_t)i + 2] = tris[i].v2_idx;
    t[4 * (size_t)i + 3] = tri_slot ? tri_slot[i] : i;
  }
  return t;
}

}  // namespace scene_refit
}  // namespace srt
