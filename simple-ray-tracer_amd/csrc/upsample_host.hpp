// upsample_host.hpp -- host-only parts of the guided upsampler (include/srt_upsample.h): parameter validation, the
// sizes and the launch of a factor, the kernel variant, and the integer axis terms of the contract (the kernel states
// them again in upsample.hpp; tests/cpp/test_upsample_host.cpp holds this copy to the contract's tables).  No device,
// no HIP header: that test links upsample_host.cpp alone.
#pragma once

#include <cstddef>
#include <cstdint>

#include "../../include/srt_upsample.h"

namespace srt {
namespace upsample {

constexpr int kBlock = 256;             // lanes per block
constexpr int kTileW = 32, kTileH = 8;  // full-resolution pixels of a block, one per lane
constexpr int kStagedBytes = 32;        // LDS per staged low pixel: colour | id and normal | t, a float4 each
constexpr int kMaxDim = 65535;          // the denoiser's image limits, applied to the full size
constexpr uint64_t kMaxPixels = 1ull << 28;

srt_upsample_params DefaultParams();
// SRT_OK, or SRT_ERR_INVALID: NULL, normal_squarings past 8, a sigma_depth that is not finite and > 0.
int ValidateParams(const srt_upsample_params* p);

// floor(n / d) for d > 0 and n >= -d.
constexpr int FloorDiv(int n, int d) { return (n + d) / d - 1; }

// The axis terms of full coordinate X at factor f: n = 2X + 1 - f, i0 = floor(n / 2f), r = n - 2f * i0,
// a1 = float(r) / float(2f), a0 = 1.0f - a1.
struct Axis {
  int i0;
  float a0, a1;
};
Axis AxisTerms(int X, int f);

struct Plan {
  int low_w = 0, low_h = 0, factor = 0;
  int width = 0, height = 0;         // factor * low
  unsigned grid_x = 0, grid_y = 0;   // blocks of kTileW x kTileH full pixels
  int foot_w = 0, foot_h = 0;        // low pixels a block's taps can reach, rescue ring included
  size_t lds_bytes = 0;              // foot_w * foot_h * kStagedBytes (the staged variant)
};
// SRT_OK; SRT_ERR_INVALID for a NULL `out`, a factor outside 1..SRT_UPSAMPLE_MAX_FACTOR or a dimension < 1;
// SRT_ERR_LIMIT for a full size past kMaxDim or kMaxPixels.
int PlanLaunch(int low_w, int low_h, int factor, Plan* out);

// The first low pixel of the footprint of the block whose first full pixel is T0 (a multiple of the tile's extent).
constexpr int FootOrigin(int T0, int f) { return FloorDiv(2 * T0 + 1 - f, 2 * f) - 1; }

// SRT_UPSAMPLE_STAGED's value (NULL: unset): "0" reads every tap from global memory, "1" stages the footprint in LDS;
// anything else is the default, kDefaultStaged (measured: tools/bench_upsample.py).
constexpr bool kDefaultStaged = true;
bool Staged(const char* env);

}  // namespace upsample
}  // namespace srt
