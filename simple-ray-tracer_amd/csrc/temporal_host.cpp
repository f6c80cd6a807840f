// temporal_host.cpp -- see temporal_host.hpp.
#include "temporal_host.hpp"

#include <cmath>

namespace srt {
namespace temporal {

srt_temporal_params DefaultParams() {
  srt_temporal_params p;
  p.max_history = 32;
  p.depth_tol = 0.05f;
  p.normal_min = 0.9f;
  return p;
}

int ValidateParams(const srt_temporal_params* p) {
  if (!p) return SRT_ERR_INVALID;
  if (p->max_history < 1 || p->max_history > (uint32_t)SRT_TEMPORAL_MAX_HISTORY) return SRT_ERR_INVALID;
  if (!std::isfinite(p->depth_tol) || !(p->depth_tol > 0.0f)) return SRT_ERR_INVALID;
  if (!std::isfinite(p->normal_min) || p->normal_min < -1.0f || p->normal_min > 1.0f) return SRT_ERR_INVALID;
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
  out->id_bytes = (size_t)pixels * 4;
  out->scratch_bytes = 2 * (out->color_bytes + out->guide_bytes + out->id_bytes);
  out->grid_x = (unsigned)((width + kRowW - 1) / kRowW);
  out->grid_y = (unsigned)((height + kRowH - 1) / kRowH);
  return SRT_OK;
}

void Reset(History* h) {
  h->valid = false;
  h->frames = 0;
}

void Advance(History* h, const srt_temporal_camera& cam) {
  h->read ^= 1;
  h->valid = true;
  h->prev = cam;
  if (h->frames < 0x7FFFFFFFu) ++h->frames;
}

}  // namespace temporal
}  // namespace srt
