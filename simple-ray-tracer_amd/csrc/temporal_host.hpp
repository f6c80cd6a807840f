// temporal_host.hpp -- host-only parts of the temporal reprojection (include/srt_temporal.h): parameter
// validation, buffer sizing, the launch grid and the ping-pong state of the history.  No device, no HIP
// header: tests/cpp/test_temporal_host.cpp links temporal_host.cpp alone.
#pragma once

#include <cstddef>
#include <cstdint>

#include "../../include/srt_temporal.h"

namespace srt {
namespace temporal {

constexpr int kBlock = 256;              // lanes per block
constexpr int kRowW = 64, kRowH = 4;     // pixels of a block: a wave is 64 contiguous pixels of one row
constexpr int kMaxDim = 65535;
constexpr uint64_t kMaxPixels = 1ull << 28;

srt_temporal_params DefaultParams();
// SRT_OK, or SRT_ERR_INVALID: NULL, max_history outside 1..65535, depth_tol not finite and > 0, normal_min not
// finite or outside [-1, 1].
int ValidateParams(const srt_temporal_params* p);

struct Sizes {
  uint64_t pixels = 0;
  size_t color_bytes = 0;    // one history colour buffer: float4 (rgb | N) per pixel
  size_t guide_bytes = 0;    // one packed guide: float4 (normal | t) per pixel
  size_t id_bytes = 0;       // one id array: the hit's BVH record, all ones for a miss
  size_t scratch_bytes = 0;  // two of each: the kernel reads arbitrary previous pixels while it writes
  unsigned grid_x = 0, grid_y = 0;
};
// SRT_OK; SRT_ERR_INVALID for a dimension < 1 or NULL `out`; SRT_ERR_LIMIT past kMaxDim or kMaxPixels.
int PlanBuffers(int width, int height, Sizes* out);

// The history's state: which of the two buffer sets holds the previous frame, whether it holds one at all, and
// the accumulate calls since the last reset.
struct History {
  int read = 0;        // the set the next call reads; it writes set `read ^ 1`
  bool valid = false;  // set `read` holds a previous frame (and `prev` its camera)
  uint32_t frames = 0;
  srt_temporal_camera prev = {};
};
void Reset(History* h);
inline int WriteIndex(const History& h) { return h.read ^ 1; }
// After a call was enqueued: the written set becomes the one to read, `cam` the previous camera.
void Advance(History* h, const srt_temporal_camera& cam);

}  // namespace temporal
}  // namespace srt
