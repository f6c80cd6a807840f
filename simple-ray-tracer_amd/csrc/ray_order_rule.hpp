// ray_order_rule.hpp -- the rule of include/srt_query_sort.h as code both sides compile: the bounds of a batch's ray
// origins, the key of a ray in them, and nothing else -- the order is the stable sort of 0 .. n-1 by key.
// ray_order_host.cpp (the host mirror) and query_sort.hpp (the kernels) include this one text, so the two cannot drift.
// Written as rebuild_rule.hpp is: no HIP header, no library call; selects, single fp32 operations and integer
// arithmetic only (the build's flags keep them uncontracted and the division correctly rounded).
//
// 1. Bounds.  Per axis, lo and hi are the least and the greatest origin[k] over the rays whose origin[k] is finite, in
//    the total order of the ordered() words (ordered_word.hpp), so an atomic max over words and a loop over values pick
//    the same one, signed zeros included.  Six words, zero before the first ray: ~ordered(lo) xyz, ordered(hi) xyz.  An
//    axis whose words stayed zero has no finite origin: lo = hi = 0, no extent.
// 2. Origin cell, kOriginBits bits an axis, in the shape of rebuild::Cell: ext = hi - lo,
//    u = ext > 0 ? ((o - lo) / ext) * 2^kOriginBits : 0, converted by selects -- !(u > 0) gives 0, u >= max gives max --
//    which sends NaN to 0 and overflow to the ends without an undefined conversion.
// 3. Direction cell, kDirBits bits an axis, normalised on the cube: m = max(|dx|, |dy|, |dz|) by selects (a NaN
//    component is passed over unless it is the first), r = d[k] / m, u = (r + 1) * 2^(kDirBits - 1) where m is finite and
//    above zero, else 0, and the same conversion.
// 4. Key: (Morton(origin cells) << 3 * kDirBits) | Morton(direction cells); kKeyBits bits, the origin the major part.
#pragma once

#include <cstdint>

#include "ordered_word.hpp"
#include "rebuild_rule.hpp"

#ifndef SRT_RAY_ORIGIN_BITS
#define SRT_RAY_ORIGIN_BITS 6
#endif
#ifndef SRT_RAY_DIR_BITS
#define SRT_RAY_DIR_BITS 4
#endif

namespace srt {
namespace rayorder {

constexpr int kOriginBits = SRT_RAY_ORIGIN_BITS;  // per axis
constexpr int kDirBits = SRT_RAY_DIR_BITS;        // per axis
constexpr int kKeyBits = 3 * (kOriginBits + kDirBits);
static_assert(kOriginBits >= 1 && kOriginBits <= 10 && kDirBits >= 0 && kDirBits <= 10, "Spread3 takes 10 bits");
static_assert(kKeyBits <= 32, "the key is one dword");

constexpr int kWords = 6;  // ~ordered(lo) xyz, ordered(hi) xyz

SRT_RULE_HD uint32_t Bits(float f) { return __builtin_bit_cast(uint32_t, f); }

// fabsf(x) <= FLT_MAX
SRT_RULE_HD bool Finite(float x) { return (Bits(x) & 0x7FFFFFFFu) < 0x7F800000u; }

SRT_RULE_HD float Abs(float x) { return __builtin_bit_cast(float, Bits(x) & 0x7FFFFFFFu); }

// Rule 1: one origin folded into the six words.
SRT_RULE_HD void Fold(uint32_t* w, float ox, float oy, float oz) {
  const float o[3] = {ox, oy, oz};
  for (int k = 0; k < 3; ++k) {
    const uint32_t e = rebuild::ordered(o[k]);
    const uint32_t lo = Finite(o[k]) ? ~e : 0u, hi = Finite(o[k]) ? e : 0u;
    w[k] = lo > w[k] ? lo : w[k];
    w[3 + k] = hi > w[3 + k] ? hi : w[3 + k];
  }
}

// Two sets of words in one (what the reductions do).
SRT_RULE_HD void Merge(uint32_t* w, const uint32_t* o) {
  for (int k = 0; k < kWords; ++k) w[k] = o[k] > w[k] ? o[k] : w[k];
}

struct Bounds {
  float lo[3], hi[3];
};

SRT_RULE_HD Bounds Decode(const uint32_t* w) {
  Bounds b;
  for (int k = 0; k < 3; ++k) {
    const bool any = w[3 + k] != 0u;  // (a finite origin sets both words of its axis)
    b.lo[k] = any ? rebuild::unordered(~w[k]) : 0.0f;
    b.hi[k] = any ? rebuild::unordered(w[3 + k]) : 0.0f;
  }
  return b;
}

// min((uint32_t)u, max) with a saturating conversion, as selects; NaN gives 0.
SRT_RULE_HD uint32_t Quantize(float u, uint32_t max) {
  return !(u > 0.0f) ? 0u : (u >= (float)max ? max : (uint32_t)u);
}

// Rule 2.
SRT_RULE_HD uint32_t OriginCell(float lo, float hi, float o) {
  const float ext = hi - lo;
  float u = 0.0f;
  if (ext > 0.0f) {
    const float r = (o - lo) / ext;
    u = r * (float)(1u << kOriginBits);
  }
  return Quantize(u, (1u << kOriginBits) - 1u);
}

// Rule 3: m of a direction, and the cell of one component.
SRT_RULE_HD float CubeNorm(float dx, float dy, float dz) {
  const float ax = Abs(dx), ay = Abs(dy), az = Abs(dz);
  float m = ax;
  m = ay > m ? ay : m;
  m = az > m ? az : m;
  return m;
}

SRT_RULE_HD uint32_t DirCell(float m, float d) {
  const float r = d / m;
  const float v = (r + 1.0f) * (0.5f * (float)(1u << kDirBits));
  const float u = ((m > 0.0f) & Finite(m)) ? v : 0.0f;
  return Quantize(u, (1u << kDirBits) - 1u);
}

// Rule 4.
SRT_RULE_HD uint32_t Key(const Bounds& b, float ox, float oy, float oz, float dx, float dy, float dz) {
  const uint32_t qo = rebuild::Morton(OriginCell(b.lo[0], b.hi[0], ox), OriginCell(b.lo[1], b.hi[1], oy),
                                      OriginCell(b.lo[2], b.hi[2], oz));
  const float m = CubeNorm(dx, dy, dz);
  const uint32_t qd = rebuild::Morton(DirCell(m, dx), DirCell(m, dy), DirCell(m, dz));
  return (qo << (3 * kDirBits)) | qd;
}

}  // namespace rayorder
}  // namespace srt
