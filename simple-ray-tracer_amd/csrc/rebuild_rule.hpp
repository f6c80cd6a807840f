// rebuild_rule.hpp -- the rule of include/srt_rebuild.h as code both sides compile: the key of a triangle, the
// common prefix of two positions and one node of Karras' hierarchy.  rebuild_host.cpp (the host mirror) and
// rebuild.hpp (the kernels) include this one text, so the two cannot drift.  No HIP header, no library call: selects,
// single fp32 operations and integer arithmetic only (the build's flags keep them uncontracted and the division
// correctly rounded).
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define SRT_RULE_HD __host__ __device__ inline
#else
#define SRT_RULE_HD inline
#endif

namespace srt {
namespace rebuild {

constexpr uint32_t kMaxTris = 1u << 30;  // the hierarchy's position arithmetic and the depth bound hold below
constexpr int kHeightBins = 64;          // heights <= depth <= 30 + ceil(log2 n) <= 60 for n < 2^30

// Rule 2, one component: the 10-bit cell of a triangle whose vertices span [bmin, bmax] in a scene box [lo, hi].
SRT_RULE_HD uint32_t Cell(float lo, float hi, float bmin, float bmax) {
  const float c = 0.5f * (bmin + bmax);
  const float ext = hi - lo;
  float u = 0.0f;
  if (ext > 0.0f) {
    const float r = (c - lo) / ext;
    u = r * 1024.0f;
  }
  // min((uint32_t)u, 1023u) with a saturating conversion, as selects
  return !(u > 0.0f) ? 0u : (u >= 1023.0f ? 1023u : (uint32_t)u);
}

// 10 bits spread to every third bit.
SRT_RULE_HD uint32_t Spread3(uint32_t x) {
  x = (x * 0x00010001u) & 0xFF0000FFu;
  x = (x * 0x00000101u) & 0x0F00F00Fu;
  x = (x * 0x00000011u) & 0xC30C30C3u;
  x = (x * 0x00000005u) & 0x49249249u;
  return x;
}

SRT_RULE_HD uint32_t Morton(uint32_t qx, uint32_t qy, uint32_t qz) {
  return (Spread3(qx) << 2) | (Spread3(qy) << 1) | Spread3(qz);
}

// Rule 4: the common prefix of positions i and j of the sorted keys; -1 when j lies outside [0, n).
SRT_RULE_HD int Prefix(const uint32_t* keys, int64_t n, int64_t i, int64_t j) {
  if (j < 0 || j >= n) return -1;
  const uint32_t x = keys[i] ^ keys[j];
  if (x != 0u) return __builtin_clz(x);
  const uint32_t y = (uint32_t)i ^ (uint32_t)j;
  return y != 0u ? 32 + __builtin_clz(y) : 64;
}

// A child reference of the hierarchy: leaf position or internal node index.
struct Child {
  uint32_t index;
  bool leaf;
};

// Internal node i (0 <= i < n - 1, n >= 2) of Karras' binary radix tree over keys[0 .. n): its range is [i, j] or
// [j, i], split after position `gamma`; the left child covers the lower positions.
SRT_RULE_HD void KarrasNode(const uint32_t* keys, int64_t n, int64_t i, Child* left, Child* right) {
  const int d = Prefix(keys, n, i, i + 1) - Prefix(keys, n, i, i - 1) < 0 ? -1 : 1;
  const int floor_prefix = Prefix(keys, n, i, i - d);
  int64_t lmax = 2;
  while (Prefix(keys, n, i, i + lmax * d) > floor_prefix) lmax *= 2;  // (ends: positions outside give -1)
  int64_t l = 0;
  for (int64_t t = lmax / 2; t >= 1; t /= 2)
    if (Prefix(keys, n, i, i + (l + t) * d) > floor_prefix) l += t;
  const int64_t j = i + l * d;
  const int node_prefix = Prefix(keys, n, i, j);
  int64_t s = 0;
  for (int64_t t = (l + 1) / 2;; t = (t + 1) / 2) {
    if (Prefix(keys, n, i, i + (s + t) * d) > node_prefix) s += t;
    if (t <= 1) break;
  }
  const int64_t gamma = i + s * d + (d < 0 ? -1 : 0);
  const int64_t first = i < j ? i : j, last = i < j ? j : i;
  left->index = (uint32_t)gamma;
  left->leaf = first == gamma;
  right->index = (uint32_t)(gamma + 1);
  right->leaf = last == gamma + 1;
}

}  // namespace rebuild
}  // namespace srt
