// refit_levels.hpp -- the levels of a refit schedule, for every schedule the project makes: the query refit's pairs
// (refit_host.cpp), the path tracer's node slots (scene_refit_host.cpp) and the rebuild's pairs, whose counts per
// height the device reports (rebuild_host.cpp).  Entries go bottom-up by height; a height's entries are
// order[first[h] .. first[h+1]).  Heights below `tail_begin` get a launch each; the maximal suffix of heights that
// each hold at most kBlock entries runs in one block.  Host only and header only: no HIP header, nothing to link.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace srt {
namespace refit {

constexpr uint32_t kBlock = 256;  // lanes per block of the refit kernels; a height of at most this many entries fuses

struct Levels {
  std::vector<uint32_t> first;  // heights + 1 entries
  uint32_t heights = 0;
  uint32_t tail_begin = 0;      // first height of the one-block tail (== heights when none fuses)
  uint32_t launches = 0;        // the triangle kernel (where the caller counts one) + tail_begin + the tail
};

// Closes `l` over counts[h] entries at height h < heights: the offsets, the tail rule, the launches.
inline void CloseLevels(const uint32_t* counts, uint32_t heights, bool tris_launch, Levels* l) {
  l->heights = heights;
  l->first.assign((size_t)heights + 1, 0);
  for (uint32_t h = 0; h < heights; ++h) l->first[h + 1] = l->first[h] + counts[h];
  l->tail_begin = heights;
  while (l->tail_begin > 0 && l->first[l->tail_begin] - l->first[l->tail_begin - 1] <= kBlock) --l->tail_begin;
  l->launches = (tris_launch ? 1u : 0u) + l->tail_begin + 1;
}

constexpr uint32_t kNoHeight = 0xFFFFFFFFu;  // an index the schedule leaves out

// The counting sort by height: closes `l` over height[i] (kNoHeight: skipped) and fills `order` with entry(i),
// ascending i inside a height.
template <class Entry, class Make>
void SortByHeight(const std::vector<uint32_t>& height, bool tris_launch, Make entry, Levels* l, std::vector<Entry>* order) {
  uint32_t heights = 0;
  for (uint32_t h : height)
    if (h != kNoHeight) heights = std::max(heights, h + 1);
  std::vector<uint32_t> at(heights, 0);
  for (uint32_t h : height)
    if (h != kNoHeight) ++at[h];
  CloseLevels(at.data(), heights, tris_launch, l);
  at.assign(l->first.begin(), l->first.end() - 1);
  order->resize(l->first[heights]);
  for (uint32_t i = 0; i < (uint32_t)height.size(); ++i)
    if (height[i] != kNoHeight) (*order)[at[height[i]]++] = entry(i);
}

}  // namespace refit
}  // namespace srt
