// upsample.hip -- the guided upsampler of include/srt_upsample.h: the object and the launch of upsample.hpp's
// kernel with upsample_host.hpp's plan.  A translation unit of its own, as denoise.hip is: pathtrace.hip and its
// headers (the device code srt_code_hash identifies) are only read.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>
#include <string>

#include "../../include/srt_upsample.h"
#include "stage.hpp"
#include "upsample.hpp"
#include "upsample_host.hpp"

using srt::stage::Aligned;

struct srt_upsampler : srt::stage::Stage {
  srt::upsample::Plan plan;
  srt_upsample_params params;
  bool staged = true;
  int last_launches = 0;
};

extern "C" {

int srt_upsample_abi_version(void) { return SRT_UPSAMPLE_ABI_VERSION; }

int srt_upsample_create(int device, void* stream, int low_w, int low_h, int factor, srt_upsampler** out) {
  if (!out) return SRT_ERR_INVALID;
  *out = nullptr;
  srt::upsample::Plan plan;
  if (int rc = srt::upsample::PlanLaunch(low_w, low_h, factor, &plan)) {  // before any device is touched
    srt::SetError(rc == SRT_ERR_LIMIT
                      ? "srt_upsample_create: full image past 65535 in a dimension or 2^28 pixels"
                      : "srt_upsample_create: factor must be 1..4, low_w and low_h at least 1");
    return rc;
  }
  srt::stage::Owned<srt_upsampler> up(new srt_upsampler());
  up->plan = plan;
  up->params = srt::upsample::DefaultParams();
  up->staged = srt::upsample::Staged(std::getenv("SRT_UPSAMPLE_STAGED"));
  if (int rc = up->Acquire(device, stream)) return rc;
  *out = up.release();
  return SRT_OK;
}

int srt_upsample_destroy(srt_upsampler* up) {
  if (!up) return SRT_ERR_INVALID;
  srt::stage::Destroy()(up);
  return SRT_OK;
}

void* srt_upsample_stream(srt_upsampler* up) { return srt::stage::StreamOf(up); }

int srt_upsample_get_int(srt_upsampler* up, const char* name, int* v) {
  if (!up || !name || !v) return SRT_ERR_INVALID;
  const std::string n(name);
  if (n == "factor") *v = up->plan.factor;
  else if (n == "low.width") *v = up->plan.low_w;
  else if (n == "low.height") *v = up->plan.low_h;
  else if (n == "width") *v = up->plan.width;
  else if (n == "height") *v = up->plan.height;
  else if (n == "launches") *v = up->last_launches;
  else if (n == "scratch.bytes") *v = 0;
  else if (n == "launch.blocks") *v = srt::stage::SaturateInt((size_t)up->plan.grid_x * (size_t)up->plan.grid_y);
  else if (n == "launch.block") *v = srt::upsample::kBlock;
  else return SRT_ERR_NOT_FOUND;
  return SRT_OK;
}

int srt_upsample_get_params(srt_upsampler* up, srt_upsample_params* p) {
  if (!up || !p) return SRT_ERR_INVALID;
  *p = up->params;
  return SRT_OK;
}

int srt_upsample_set_params(srt_upsampler* up, const srt_upsample_params* p) {
  if (!up) return SRT_ERR_INVALID;
  if (int rc = srt::upsample::ValidateParams(p)) {
    srt::SetError("srt_upsample_set_params: normal_squarings 0..8, sigma_depth finite and > 0");
    return rc;
  }
  up->params = *p;
  return SRT_OK;
}

int srt_upsample_run(srt_upsampler* up, const void* low_accum_dev, int frames, const srt_hit* low_guide_dev,
                     const srt_hit* full_guide_dev, void* out_rgba32f_dev, void* out_rgba8_dev) {
  if (!up || !low_accum_dev || !low_guide_dev || !full_guide_dev || frames < 1 || (!out_rgba32f_dev && !out_rgba8_dev)) {
    srt::SetError("srt_upsample_run: the object, accum and both guides must not be NULL, frames at least 1, and "
                  "one output not NULL");
    return SRT_ERR_INVALID;
  }
  if (!Aligned(low_accum_dev, 16) || !Aligned(low_guide_dev, 16) || !Aligned(full_guide_dev, 16) ||
      !Aligned(out_rgba32f_dev, 16) || !Aligned(out_rgba8_dev, 4)) {
    srt::SetError("srt_upsample_run: accum, the guides and out_rgba32f must be 16-byte aligned, out_rgba8 4-byte");
    return SRT_ERR_INVALID;
  }
  STAGE_HIP_OK(hipSetDevice(up->device));
  const srt::upsample::Plan& pl = up->plan;
  srt::upsample::UParams kp;
  std::memset(&kp, 0, sizeof kp);
  kp.src = static_cast<const float4*>(low_accum_dev);
  kp.low_hits = reinterpret_cast<const uint4*>(low_guide_dev);
  kp.full_hits = reinterpret_cast<const uint4*>(full_guide_dev);
  kp.out32 = static_cast<float4*>(out_rgba32f_dev);
  kp.out8 = static_cast<uint32_t*>(out_rgba8_dev);
  kp.w = pl.low_w;
  kp.h = pl.low_h;
  kp.W = pl.width;
  kp.H = pl.height;
  kp.f = pl.factor;
  kp.foot_w = pl.foot_w;
  kp.foot_h = pl.foot_h;
  kp.nsq = (int)up->params.normal_squarings;
  kp.frames = (float)frames;
  kp.sigma_d = up->params.sigma_depth;
  const dim3 grid(pl.grid_x, pl.grid_y);
  if (up->staged)
    hipLaunchKernelGGL(srt::upsample::upsample_kernel<true>, grid, dim3(srt::upsample::kBlock), pl.lds_bytes, up->stream, kp);
  else
    hipLaunchKernelGGL(srt::upsample::upsample_kernel<false>, grid, dim3(srt::upsample::kBlock), 0, up->stream, kp);
  STAGE_HIP_OK(hipGetLastError());
  up->last_launches = SRT_UPSAMPLE_LAUNCHES;
  return SRT_OK;
}

}  // extern "C"
