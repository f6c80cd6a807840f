// denoise_host.hpp -- host-only parts of the denoiser (include/srt_denoise.h): parameter validation, buffer
// sizing, the per-pass schedule (step, sigma_color, which kernel, which buffers) and the camera basis of
// the primary rays.  No device, no HIP header: tests/cpp/test_denoise_host.cpp links denoise_host.cpp alone.
#pragma once

#include <cstddef>
#include <cstdint>

#include "../../include/srt_denoise.h"
#include "../../include/srt_variance.h"

namespace srt {
namespace denoise {

constexpr int kBlock = 256;              // lanes per block of every denoise kernel
constexpr int kTileW = 32, kTileH = 8;   // pixels of a block of the LDS-tiled kernel (one per lane)
constexpr int kDirectW = 64, kDirectH = 4;  // pixels of a block of the direct kernel: a wave is 64 pixels of a row
constexpr int kStagedBytes = 32;         // LDS per staged pixel: colour | id and normal | t, a float4 each
// The tile plus its halo of 2 * step pixels must fit a block's LDS: step 8 stages 64 x 40 pixels (80 KiB),
// step 16 would need 216 KiB of the CU's 160.
constexpr int kTileStepLimit = 8;
// LDS is handed out in 128 units of 1280 B per CU.  Step 1 stages 36 x 12 pixels = 11 units and step 2
// 40 x 16 = exactly 16, so 8 blocks (all 32 waves) still share a CU; step 4 needs 29 units and halves that.
// Default crossover, measured (tools/bench_denoise.py, profiles/denoise.json, 1920x1080): the tiled kernel wins
// at step 1 only (59 against 82 us, where it also shares the first pass's three loads per pixel); from step 2
// on the direct kernel is as fast or faster (51-53 against 53-54 us at step 2, 50 against 64 at 4, 47 against
// 162 at 8).  SRT_DENOISE_TILE overrides it ("Denoiser").
constexpr int kDefaultTileMaxStep = 1;
constexpr size_t kLdsUnit = 160 * 1024 / 128;
constexpr int kMaxDim = 65535;
constexpr uint64_t kMaxPixels = 1ull << 28;

srt_denoise_params DefaultParams();
// SRT_OK, or SRT_ERR_INVALID: NULL, passes or normal_squarings past 8, a sigma that is not finite and > 0.
int ValidateParams(const srt_denoise_params* p);

struct Sizes {
  uint64_t pixels = 0;
  size_t color_bytes = 0;    // one ping-pong colour buffer: float4 (colour | id) per pixel
  size_t guide_bytes = 0;    // the packed guide: float4 (normal | t) per pixel
  size_t scratch_bytes = 0;  // two colour buffers + the guide
};
// SRT_OK; SRT_ERR_INVALID for a dimension < 1 or NULL `out`; SRT_ERR_LIMIT past kMaxDim or kMaxPixels.
int PlanBuffers(int width, int height, Sizes* out);

// SRT_DENOISE_TILE's value (NULL: unset) as the largest tiled step: a power of two in 0..kTileStepLimit
// (other values round down; 0 = every pass direct, 8 = every pass that can be tiled is).
int TileMaxStep(const char* env);
// LDS of a tiled block at `step`, and the same in whole allocation units.
size_t TileLdsBytes(int step);
size_t TileLdsUnits(int step);

// Image a pass reads or writes.
enum Buf : int { kAccum = -1, kPing = 0, kPong = 1, kOutput = 2 };
struct Pass {
  int step = 1;
  float sigma_c = 0.0f;   // sigma_color * 2^-i
  bool tiled = false;
  size_t lds_bytes = 0;   // dynamic LDS of the launch (0: direct)
  bool first = false;     // reads the accumulation image and the srt_hit records; writes the packed guide
  bool last = false;      // writes the outputs instead of a colour buffer
  int src = kAccum, dst = kOutput;
  unsigned grid_x = 0, grid_y = 0;
};
// Fills out[0 .. passes - 1] and returns `passes`.
int BuildSchedule(const srt_denoise_params& p, int tile_max_step, int width, int height,
                  Pass out[SRT_DENOISE_MAX_PASSES]);

// ---- the variance-guided filter (include/srt_variance.h) ----

srt_denoise_var_params DefaultVarParams();
// SRT_OK, or SRT_ERR_INVALID: NULL, sigma_lum not finite and > 0, min_history outside 1..65535.
int ValidateVarParams(const srt_denoise_var_params* p);
// One variance array: a float per pixel.  The object holds two; they are no part of Sizes::scratch_bytes.
inline size_t VarianceBytes(const Sizes& s) { return (size_t)s.pixels * 4; }

// A launch of srt_denoise_run_variance.  Launch 0 is the resolve (mean, guide pack, var_0) into set 0 of the
// ping-pong colour and variance buffers; launch 1 + i is pass i, reading set i & 1 and writing the other, the
// last one the outputs.  Every launch has the direct kernel's shape (kDirectW x kDirectH pixels a block).
struct VarLaunch {
  bool resolve = false;
  bool last = false;
  int step = 0;            // 2^i (0 for the resolve)
  int src = kAccum, dst = kOutput;
  unsigned grid_x = 0, grid_y = 0;
};
// Fills out[0 .. passes] and returns 1 + passes, or 0 when passes == 0 (the variance filter needs a pass).
int BuildVarianceSchedule(const srt_denoise_params& p, int width, int height, VarLaunch out[SRT_DENOISE_MAX_PASSES + 1]);

// du = right / W, dv = up / H, p00 = (o + front - right/2 - up/2) + 0.5 * (du + dv); fp32, in that order.
struct Basis {
  float o[3], p00[3], du[3], dv[3];
};
void PrimaryBasis(const float origin[3], const float front[3], const float right[3], const float up[3], int width,
                  int height, Basis* out);

}  // namespace denoise
}  // namespace srt
