// ray_order_host.cpp -- see ray_order_host.hpp.
#include "ray_order_host.hpp"

#include <algorithm>
#include <climits>
#include <numeric>
#include <vector>

#include "ray_order_rule.hpp"

namespace srt {
namespace rayorder {

int RayOrder(const srt_ray* rays, uint32_t n, uint32_t* order, uint32_t* keys, float* bounds, std::string* err) {
  if ((n && (!rays || !order))) {
    if (err) *err = "srt_ray_order: null rays or order";
    return SRT_ERR_INVALID;
  }
  uint32_t words[kWords] = {};
  for (uint32_t i = 0; i < n; ++i) Fold(words, rays[i].origin[0], rays[i].origin[1], rays[i].origin[2]);
  const Bounds b = Decode(words);
  if (bounds)
    for (int k = 0; k < 3; ++k) {
      bounds[k] = b.lo[k];
      bounds[3 + k] = b.hi[k];
    }
  if (n == 0) return SRT_OK;
  std::vector<uint32_t> key(n);
  for (uint32_t i = 0; i < n; ++i) {
    const srt_ray& r = rays[i];
    key[i] = Key(b, r.origin[0], r.origin[1], r.origin[2], r.direction[0], r.direction[1], r.direction[2]);
  }
  std::iota(order, order + n, 0u);
  std::stable_sort(order, order + n, [&](uint32_t a, uint32_t c) { return key[a] < key[c]; });
  if (keys)
    for (uint32_t i = 0; i < n; ++i) keys[i] = key[order[i]];
  return SRT_OK;
}

int CheckSorted(uint32_t n, std::string* err) {
  if (n > (uint32_t)INT_MAX) {
    if (err) *err = "srt_query sorted call: more than INT_MAX rays (the device sort counts in int)";
    return SRT_ERR_INVALID;
  }
  return SRT_OK;
}

int OriginBits() { return kOriginBits; }
int DirBits() { return kDirBits; }
int KeyBits() { return kKeyBits; }

}  // namespace rayorder
}  // namespace srt
