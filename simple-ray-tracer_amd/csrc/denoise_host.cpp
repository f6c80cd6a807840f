// denoise_host.cpp -- see denoise_host.hpp.
#include "denoise_host.hpp"

#include <cmath>
#include <cstdlib>

namespace srt {
namespace denoise {

srt_denoise_params DefaultParams() {
  // sigmas: the lowest MSE of tools/denoise_sigma_grid.py's grid ("Denoiser")
  srt_denoise_params p;
  p.passes = 5;
  p.normal_squarings = 5;
  p.sigma_color = 3.0f;
  p.sigma_depth = 0.2f;
  return p;
}

int ValidateParams(const srt_denoise_params* p) {
  if (!p) return SRT_ERR_INVALID;
  if (p->passes > SRT_DENOISE_MAX_PASSES || p->normal_squarings > SRT_DENOISE_MAX_NORMAL_SQUARINGS) return SRT_ERR_INVALID;
  if (!std::isfinite(p->sigma_color) || !(p->sigma_color > 0.0f)) return SRT_ERR_INVALID;
  if (!std::isfinite(p->sigma_depth) || !(p->sigma_depth > 0.0f)) return SRT_ERR_INVALID;
  return SRT_OK;
}

int PlanBuffers(int width, int height, Sizes* out) {
  if (!out) return SRT_ERR_INVALID;
  *out = Sizes();
  if (width < 1 || height < 1) return SRT_ERR_INVALID;
  const uint64_t pixels = (uint64_t)width * (uint64_t)height;
  if (width > kMaxDim || height > kMaxDim || pixels > kMaxPixels) return SRT_ERR_LIMIT;
  out->pixels = pixels;
  out->color_bytes = (size_t)pixels * 16;
  out->guide_bytes = (size_t)pixels * 16;
  out->scratch_bytes = 2 * out->color_bytes + out->guide_bytes;
  return SRT_OK;
}

int TileMaxStep(const char* env) {
  if (!env || !*env) return kDefaultTileMaxStep;
  const long v = std::strtol(env, nullptr, 10);
  int step = 0;
  for (int s = 1; s <= kTileStepLimit && s <= v; s *= 2) step = s;
  return step;
}

size_t TileLdsBytes(int step) {
  return (size_t)(kTileW + 4 * step) * (size_t)(kTileH + 4 * step) * kStagedBytes;
}

size_t TileLdsUnits(int step) { return (TileLdsBytes(step) + kLdsUnit - 1) / kLdsUnit; }

int BuildSchedule(const srt_denoise_params& p, int tile_max_step, int width, int height,
                  Pass out[SRT_DENOISE_MAX_PASSES]) {
  const int n = (int)(p.passes < (uint32_t)SRT_DENOISE_MAX_PASSES ? p.passes : (uint32_t)SRT_DENOISE_MAX_PASSES);
  for (int i = 0; i < n; ++i) {
    Pass& q = out[i];
    q = Pass();
    q.step = 1 << i;
    q.sigma_c = p.sigma_color * std::ldexp(1.0f, -i);
    q.tiled = q.step <= tile_max_step && q.step <= kTileStepLimit;
    q.lds_bytes = q.tiled ? TileLdsBytes(q.step) : 0;
    q.first = i == 0;
    q.last = i == n - 1;
    q.src = q.first ? kAccum : ((i - 1) & 1);
    q.dst = q.last ? kOutput : (i & 1);
    const int bw = q.tiled ? kTileW : kDirectW, bh = q.tiled ? kTileH : kDirectH;
    q.grid_x = (unsigned)((width + bw - 1) / bw);
    q.grid_y = (unsigned)((height + bh - 1) / bh);
  }
  return n;
}

srt_denoise_var_params DefaultVarParams() {
  // sigma_lum: the lowest tone-mapped MSE of tools/variance_sigma_grid.py's grid at 5 passes, summed over its two
  // sequences ("Variance-guided filter"); SVGF's own 4 was the starting point
  srt_denoise_var_params p;
  p.sigma_lum = 1.0f;
  p.min_history = 4;
  return p;
}

int ValidateVarParams(const srt_denoise_var_params* p) {
  if (!p) return SRT_ERR_INVALID;
  if (!std::isfinite(p->sigma_lum) || !(p->sigma_lum > 0.0f)) return SRT_ERR_INVALID;
  if (p->min_history < 1 || p->min_history > (uint32_t)SRT_VARIANCE_MAX_MIN_HISTORY) return SRT_ERR_INVALID;
  return SRT_OK;
}

int BuildVarianceSchedule(const srt_denoise_params& p, int width, int height, VarLaunch out[SRT_DENOISE_MAX_PASSES + 1]) {
  const int n = (int)(p.passes < (uint32_t)SRT_DENOISE_MAX_PASSES ? p.passes : (uint32_t)SRT_DENOISE_MAX_PASSES);
  if (n == 0) return 0;
  for (int l = 0; l <= n; ++l) {
    VarLaunch& q = out[l];
    q = VarLaunch();
    q.resolve = l == 0;
    q.last = l == n;
    q.step = l == 0 ? 0 : 1 << (l - 1);
    q.src = l == 0 ? kAccum : ((l - 1) & 1);
    q.dst = q.last ? kOutput : (l & 1);
    q.grid_x = (unsigned)((width + kDirectW - 1) / kDirectW);
    q.grid_y = (unsigned)((height + kDirectH - 1) / kDirectH);
  }
  return n + 1;
}

void PrimaryBasis(const float origin[3], const float front[3], const float right[3], const float up[3], int width,
                  int height, Basis* out) {
  const float w = (float)width, h = (float)height;
  for (int k = 0; k < 3; ++k) {
    out->o[k] = origin[k];
    out->du[k] = right[k] / w;
    out->dv[k] = up[k] / h;
    const float corner = ((origin[k] + front[k]) - right[k] / 2.0f) - up[k] / 2.0f;
    const float half = out->du[k] + out->dv[k];
    out->p00[k] = corner + 0.5f * half;
  }
}

}  // namespace denoise
}  // namespace srt
