// scene_refit_host.cpp -- see scene_refit_host.hpp.
#include "scene_refit_host.hpp"

#include <algorithm>

namespace srt {
namespace scene_refit {

bool BuildSchedule(const uint32_t* ref, const uint32_t* cnt, uint32_t n_slots, uint32_t ref_or, const uint32_t* roots,
                   uint32_t n_roots, const uint32_t* tri_of_slot, uint32_t n_tri_slots, uint32_t n_tris, Schedule* out) {
  Schedule s;
  constexpr uint32_t kUnknown = refit::kNoHeight, kOpen = 0xFFFFFFFEu;
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
  auto entry = [&](uint32_t i) { return Entry{i, cnt[i] > 0 ? (tri_of_slot ? tri_of_slot[ref[i]] : ref[i]) : 0u}; };
  refit::SortByHeight(height, n_tris > 0, entry, &s, &s.order);  // (the slots no root reaches stay kUnknown)
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
