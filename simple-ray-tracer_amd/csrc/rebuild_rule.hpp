// rebuild_rule.hpp -- the rule of include/srt_rebuild.h and include/srt_rebuild_leaf.h as code both sides compile: the
// key of a triangle, the common prefix of two positions, one node of Karras' hierarchy and the collapse of its subtrees.  rebuild_host.cpp (the host mirror) and
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
// [j, i] -- positions first .. last -- split after position `gamma`; the left child covers the lower positions.
struct Split {
  int64_t first, last, gamma;
};

SRT_RULE_HD Split KarrasSplit(const uint32_t* keys, int64_t n, int64_t i) {
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
  Split sp;
  sp.gamma = i + s * d + (d < 0 ? -1 : 0);
  sp.first = i < j ? i : j;
  sp.last = i < j ? j : i;
  return sp;
}

// Rule 4 with one-triangle leaves: the two children of internal node i.
SRT_RULE_HD void KarrasNode(const uint32_t* keys, int64_t n, int64_t i, Child* left, Child* right) {
  const Split sp = KarrasSplit(keys, n, i);
  left->index = (uint32_t)sp.gamma;
  left->leaf = sp.first == sp.gamma;
  right->index = (uint32_t)(sp.gamma + 1);
  right->leaf = sp.last == sp.gamma + 1;
}

// Rule 4a (include/srt_rebuild_leaf.h): an internal node survives iff its range holds more than max_leaf positions,
// and a child range [a, b] of a surviving node is one leaf (a, b - a + 1) iff it holds at most max_leaf; otherwise it
// is the internal node `a` (a right child) or `b` (a left child), which Karras' numbering puts at the split.
constexpr uint32_t kMaxLeafLimit = 255;  // leaf counts stay below 256: PlanStack's 2-dword packing

SRT_RULE_HD bool Survives(const Split& sp, uint32_t max_leaf) { return sp.last - sp.first + 1 > (int64_t)max_leaf; }

struct Slot {
  uint32_t index;  // a leaf's first position, or the Karras index of an internal node
  uint32_t count;  // a leaf's triangles; 0: internal
};

SRT_RULE_HD Slot LeftSlot(const Split& sp, uint32_t max_leaf) {
  const int64_t c = sp.gamma - sp.first + 1;
  return c <= (int64_t)max_leaf ? Slot{(uint32_t)sp.first, (uint32_t)c} : Slot{(uint32_t)sp.gamma, 0u};
}

SRT_RULE_HD Slot RightSlot(const Split& sp, uint32_t max_leaf) {
  const int64_t c = sp.last - sp.gamma;
  return c <= (int64_t)max_leaf ? Slot{(uint32_t)(sp.gamma + 1), (uint32_t)c} : Slot{(uint32_t)(sp.gamma + 1), 0u};
}

// include/srt_rebuild_models.h: record r owns the positions [s, s + c) of the (record, key) order.  Inside a segment the
// hierarchy is the single-model rule on the segment's own keys and local positions -- a position outside the segment has
// prefix -1, equal keys tie-break by 32 + clz((i - s) ^ (j - s)) -- so node i (s <= i < s + c - 1) is KarrasSplit over
// keys + s with local index i - s, moved back to global positions.  Pair and node indices are global: node i is pair i.
SRT_RULE_HD Split SegmentSplit(const uint32_t* keys, uint32_t s, uint32_t c, uint32_t i) {
  Split sp = KarrasSplit(keys + s, (int64_t)c, (int64_t)(i - s));
  sp.first += s;
  sp.last += s;
  sp.gamma += s;
  return sp;
}

// The root reference of a record with c >= 1 positions from s: a leaf (s, c) when c <= max_leaf (c == 1 always is), else
// Karras' node s, count 0.
SRT_RULE_HD Slot SegmentRoot(uint32_t s, uint32_t c, uint32_t max_leaf) {
  return c <= max_leaf ? Slot{s, c} : Slot{s, 0u};
}

// The two keys of the (record, key) order in one: records in the high dword.
SRT_RULE_HD uint64_t RecordKey(uint32_t record, uint32_t morton) { return ((uint64_t)record << 32) | morton; }

}  // namespace rebuild
}  // namespace srt
