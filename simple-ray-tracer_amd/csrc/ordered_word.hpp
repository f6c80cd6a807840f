// ordered_word.hpp -- the order-preserving map between fp32 values and uint32 words, for both sides: a < b as floats
// (-0 below +0, negative NaNs below everything, positive NaNs above) iff ordered(a) < ordered(b) as unsigned words.  An
// atomic max over ordered(x) is the maximum of the values, over ~ordered(x) their minimum, both exact and commutative;
// no finite value maps to the word 0 either way, so a zeroed word reads as "nothing folded yet".  rebuild.hpp (the
// per-record boxes) and the ray ordering (ray_order_rule.hpp: the origin bounds, on the device and in the host mirror)
// share this one text.
#pragma once

#include <cstdint>

#include "rebuild_rule.hpp"

namespace srt {
namespace rebuild {

SRT_RULE_HD uint32_t ordered(float f) {
  const uint32_t u = __builtin_bit_cast(uint32_t, f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

SRT_RULE_HD float unordered(uint32_t e) {
  return __builtin_bit_cast(float, (e & 0x80000000u) ? (e ^ 0x80000000u) : ~e);
}

}  // namespace rebuild
}  // namespace srt
