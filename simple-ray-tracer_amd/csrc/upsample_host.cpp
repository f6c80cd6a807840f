// upsample_host.cpp -- see upsample_host.hpp.
#include "upsample_host.hpp"

#include <cmath>

namespace srt {
namespace upsample {

srt_upsample_params DefaultParams() {
  // the denoiser's values ("Denoiser")
  srt_upsample_params p;
  p.normal_squarings = 5;
  p.sigma_depth = 0.2f;
  return p;
}

int ValidateParams(const srt_upsample_params* p) {
  if (!p) return SRT_ERR_INVALID;
  if (p->normal_squarings > SRT_DENOISE_MAX_NORMAL_SQUARINGS) return SRT_ERR_INVALID;
  if (!std::isfinite(p->sigma_depth) || !(p->sigma_depth > 0.0f)) return SRT_ERR_INVALID;
  return SRT_OK;
}

Axis AxisTerms(int X, int f) {
  const int n = 2 * X + 1 - f;
  Axis a;
  a.i0 = FloorDiv(n, 2 * f);
  const int r = n - 2 * f * a.i0;
  a.a1 = (float)r / (float)(2 * f);
  a.a0 = 1.0f - a.a1;
  return a;
}

int PlanLaunch(int low_w, int low_h, int factor, Plan* out) {
  if (!out) return SRT_ERR_INVALID;
  *out = Plan();
  if (factor < 1 || factor > SRT_UPSAMPLE_MAX_FACTOR || low_w < 1 || low_h < 1) return SRT_ERR_INVALID;
  const uint64_t W = (uint64_t)low_w * (uint64_t)factor, H = (uint64_t)low_h * (uint64_t)factor;
  if (W > (uint64_t)kMaxDim || H > (uint64_t)kMaxDim || W * H > kMaxPixels) return SRT_ERR_LIMIT;
  out->low_w = low_w;
  out->low_h = low_h;
  out->factor = factor;
  out->width = (int)W;
  out->height = (int)H;
  out->grid_x = (unsigned)((out->width + kTileW - 1) / kTileW);
  out->grid_y = (unsigned)((out->height + kTileH - 1) / kTileH);
  // i0 of a tile's last pixel lies at most ceil((extent - 1) / f) past its first pixel's; the ring adds 1 before
  // and 2 after
  out->foot_w = (kTileW + factor - 1) / factor + 4;
  out->foot_h = (kTileH + factor - 1) / factor + 4;
  out->lds_bytes = (size_t)out->foot_w * (size_t)out->foot_h * kStagedBytes;
  return SRT_OK;
}

bool Staged(const char* env) {
  if (env && env[0] == '0' && !env[1]) return false;
  if (env && env[0] == '1' && !env[1]) return true;
  return kDefaultStaged;
}

}  // namespace upsample
}  // namespace srt
