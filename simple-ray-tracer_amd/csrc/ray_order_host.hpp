// ray_order_host.hpp -- the host mirror of the device ray ordering (include/srt_query_sort.h: srt_ray_order) and the
// argument checks of the sorted calls.  Pure host code over ray_order_rule.hpp, the text the kernels compile too.
#pragma once

#include <cstdint>
#include <string>

#include "../../include/srt_amd.h"

namespace srt {
namespace rayorder {

// order[n]: the stable sort of 0 .. n-1 by key.  keys[n] (sorted, keys[i] belongs to ray order[i]) and bounds[6] (lo xyz,
// hi xyz of the finite origins; zeros on an axis without one) may be null.  n == 0 writes the bounds only.
int RayOrder(const srt_ray* rays, uint32_t n, uint32_t* order, uint32_t* keys, float* bounds, std::string* err);

// What a sorted call refuses beyond what the unsorted call refuses: more rays than the device sort counts.
int CheckSorted(uint32_t n, std::string* err);

int OriginBits();
int DirBits();
int KeyBits();

}  // namespace rayorder
}  // namespace srt
