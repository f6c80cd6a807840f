// denoise.hip -- the denoiser of include/srt_denoise.h: the object, its buffers and the launches of
// denoise.hpp's kernels in denoise_host.hpp's schedule.  A translation unit of its own, as query.hip is:
// pathtrace.hip and its headers (the device code srt_code_hash identifies) are only read.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>
#include <string>

#include "../../include/srt_denoise.h"
#include "../../include/srt_variance.h"
#include "../../include/srt_surface.h"
#include "denoise.hpp"
#include "denoise_host.hpp"
#include "stage.hpp"
#include "surface_host.hpp"

using srt::stage::Aligned;
using srt::stage::DevPtr;

struct srt_denoiser : srt::stage::Stage {
  int width = 0, height = 0;
  srt::denoise::Sizes sizes;
  DevPtr<float4> d_color[2];  // ping-pong colour | id
  DevPtr<float4> d_guide;     // normal | t
  srt_denoise_params params;
  DevPtr<float> d_var[2];     // ping-pong variance (include/srt_variance.h); srt_denoise_enable_variance
  srt_denoise_var_params var_params;
  int tile_max_step = 0;
  int last_launches = 0;
};

namespace {

using srt::denoise::AParams;
using srt::denoise::DParams;
using srt::denoise::kBlock;
using srt::denoise::Pass;

int Allocate(srt_denoiser* dn) {
  STAGE_HIP_OK(srt::stage::AllocPair(dn->d_color, dn->sizes.color_bytes));
  STAGE_HIP_OK(dn->d_guide.Alloc(dn->sizes.guide_bytes));
  const size_t lds = dn->tile_max_step ? srt::denoise::TileLdsBytes(dn->tile_max_step) : 0;
  if (lds > 48 * 1024) {
    STAGE_HIP_OK(hipFuncSetAttribute((const void*)srt::denoise::denoise_tiled_kernel<true>,
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    STAGE_HIP_OK(hipFuncSetAttribute((const void*)srt::denoise::denoise_tiled_kernel<false>,
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    STAGE_HIP_OK(hipFuncSetAttribute((const void*)srt::denoise::denoise_tiled_kernel<true, AParams>,
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    STAGE_HIP_OK(hipFuncSetAttribute((const void*)srt::denoise::denoise_tiled_kernel<false, AParams>,
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  }
  return SRT_OK;
}

// One pass over P = DParams (srt_denoise_run, and the middle passes of srt_denoise_run_albedo) or AParams.
template <class P>
void LaunchPass(srt_denoiser* dn, const srt::denoise::Pass& ps, const P& dp) {
  const dim3 grid(ps.grid_x, ps.grid_y);
  if (ps.tiled) {
    if (ps.first)
      hipLaunchKernelGGL((srt::denoise::denoise_tiled_kernel<true, P>), grid, dim3(kBlock), ps.lds_bytes, dn->stream, dp);
    else
      hipLaunchKernelGGL((srt::denoise::denoise_tiled_kernel<false, P>), grid, dim3(kBlock), ps.lds_bytes, dn->stream, dp);
  } else {
    if (ps.first)
      hipLaunchKernelGGL((srt::denoise::denoise_direct_kernel<true, P>), grid, dim3(kBlock), 0, dn->stream, dp);
    else
      hipLaunchKernelGGL((srt::denoise::denoise_direct_kernel<false, P>), grid, dim3(kBlock), 0, dn->stream, dp);
  }
}

// srt_denoise_run (attrs == nullptr) and srt_denoise_run_albedo: the same schedule and launches; with attrs the
// first and the last pass are the AParams instances.
int Run(srt_denoiser* dn, const char* what, const void* accum_rgba32f_dev, int frames, const srt_hit* guide_dev,
        const srt_surface_attr* attrs, float albedo_floor, void* out_rgba32f_dev, void* out_rgba8_dev) {
  if (!dn || !accum_rgba32f_dev || frames < 1 || (!out_rgba32f_dev && !out_rgba8_dev)) return SRT_ERR_INVALID;
  if (dn->params.passes > 0 && !guide_dev) {
    srt::SetError(std::string(what) + ": a guide is needed when passes > 0");
    return SRT_ERR_INVALID;
  }
  if (!Aligned(accum_rgba32f_dev, 16) || !Aligned(guide_dev, 16) || !Aligned(out_rgba32f_dev, 16) ||
      !Aligned(out_rgba8_dev, 4)) {
    srt::SetError(std::string(what) + ": accum, guide and out_rgba32f must be 16-byte aligned, out_rgba8 4-byte");
    return SRT_ERR_INVALID;
  }
  STAGE_HIP_OK(hipSetDevice(dn->device));
  AParams dp;
  std::memset(&dp, 0, sizeof dp);
  dp.hits = reinterpret_cast<const uint4*>(guide_dev);
  dp.guide = dn->d_guide;
  dp.W = dn->width;
  dp.H = dn->height;
  dp.nsq = (int)dn->params.normal_squarings;
  dp.frames = (float)frames;
  dp.sigma_d = dn->params.sigma_depth;
  dp.attrs = reinterpret_cast<const float4*>(attrs);
  dp.floor = albedo_floor;
  float4* const out32 = static_cast<float4*>(out_rgba32f_dev);
  uint32_t* const out8 = static_cast<uint32_t*>(out_rgba8_dev);
  Pass sched[SRT_DENOISE_MAX_PASSES];
  const int n = srt::denoise::BuildSchedule(dn->params, dn->tile_max_step, dn->width, dn->height, sched);
  if (n == 0) {
    dp.src = static_cast<const float4*>(accum_rgba32f_dev);
    dp.out32 = out32;
    dp.out8 = out8;
    const unsigned blocks = (unsigned)((dn->sizes.pixels + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(srt::denoise::denoise_resolve_kernel, dim3(blocks), dim3(kBlock), 0, dn->stream,
                       static_cast<const DParams&>(dp));
    STAGE_HIP_OK(hipGetLastError());
    dn->last_launches = 1;
    return SRT_OK;
  }
  for (int i = 0; i < n; ++i) {
    const Pass& ps = sched[i];
    dp.src = ps.first ? static_cast<const float4*>(accum_rgba32f_dev) : dn->d_color[ps.src];
    dp.dst = ps.last ? nullptr : dn->d_color[ps.dst];
    dp.out32 = ps.last ? out32 : nullptr;
    dp.out8 = ps.last ? out8 : nullptr;
    dp.step = ps.step;
    dp.sigma_c = ps.sigma_c;
    if (attrs && (ps.first || ps.last))
      LaunchPass<AParams>(dn, ps, dp);
    else
      LaunchPass<DParams>(dn, ps, dp);
    STAGE_HIP_OK(hipGetLastError());
  }
  dn->last_launches = n;
  return SRT_OK;
}

}  // namespace

extern "C" {

int srt_denoise_abi_version(void) { return SRT_DENOISE_ABI_VERSION; }

int srt_denoise_create(int device, void* stream, int width, int height, srt_denoiser** out) {
  if (!out) return SRT_ERR_INVALID;
  *out = nullptr;
  srt::denoise::Sizes sizes;
  if (int rc = srt::denoise::PlanBuffers(width, height, &sizes)) {  // before any device is touched
    srt::SetError(rc == SRT_ERR_LIMIT ? "srt_denoise_create: image past 65535 in a dimension or 2^28 pixels"
                                      : "srt_denoise_create: width and height must be at least 1");
    return rc;
  }
  srt::stage::Owned<srt_denoiser> dn(new srt_denoiser());
  dn->width = width;
  dn->height = height;
  dn->sizes = sizes;
  dn->params = srt::denoise::DefaultParams();
  dn->var_params = srt::denoise::DefaultVarParams();
  dn->tile_max_step = srt::denoise::TileMaxStep(std::getenv("SRT_DENOISE_TILE"));
  if (int rc = dn->Acquire(device, stream)) return rc;
  if (int rc = Allocate(dn.get())) return rc;
  *out = dn.release();
  return SRT_OK;
}

int srt_denoise_destroy(srt_denoiser* dn) {
  if (!dn) return SRT_ERR_INVALID;
  srt::stage::Destroy()(dn);
  return SRT_OK;
}

void* srt_denoise_stream(srt_denoiser* dn) { return srt::stage::StreamOf(dn); }

int srt_denoise_get_int(srt_denoiser* dn, const char* name, int* v) {
  if (!dn || !name || !v) return SRT_ERR_INVALID;
  const std::string n(name);
  if (n == "passes") *v = (int)dn->params.passes;
  else if (n == "normal_squarings") *v = (int)dn->params.normal_squarings;
  else if (n == "width") *v = dn->width;
  else if (n == "height") *v = dn->height;
  else if (n == "scratch.bytes") *v = srt::stage::SaturateInt(dn->sizes.scratch_bytes);
  else if (n == "tile.lds_bytes") *v = dn->tile_max_step ? (int)srt::denoise::TileLdsBytes(dn->tile_max_step) : 0;
  else if (n == "tile.max_step") *v = dn->tile_max_step;
  else if (n == "tile.width") *v = srt::denoise::kTileW;
  else if (n == "tile.height") *v = srt::denoise::kTileH;
  else if (n == "launches") *v = dn->last_launches;
  else if (n == "variance.bytes") *v = srt::stage::SaturateInt(dn->d_var[0] ? 2 * srt::denoise::VarianceBytes(dn->sizes) : 0);
  else return SRT_ERR_NOT_FOUND;
  return SRT_OK;
}

int srt_denoise_get_params(srt_denoiser* dn, srt_denoise_params* p) {
  if (!dn || !p) return SRT_ERR_INVALID;
  *p = dn->params;
  return SRT_OK;
}

int srt_denoise_set_params(srt_denoiser* dn, const srt_denoise_params* p) {
  if (!dn) return SRT_ERR_INVALID;
  if (int rc = srt::denoise::ValidateParams(p)) {
    srt::SetError("srt_denoise_set_params: passes and normal_squarings 0..8, sigmas finite and > 0");
    return rc;
  }
  dn->params = *p;
  return SRT_OK;
}

int srt_denoise_primary_rays(srt_denoiser* dn, const float origin[3], const float front[3], const float right[3],
                             const float up[3], srt_ray* rays_dev) {
  if (!dn || !origin || !front || !right || !up || !rays_dev || !Aligned(rays_dev, 16)) return SRT_ERR_INVALID;
  srt::denoise::Basis b;
  srt::denoise::PrimaryBasis(origin, front, right, up, dn->width, dn->height, &b);
  srt::denoise::RayParams rp;
  rp.rays = reinterpret_cast<float4*>(rays_dev);
  rp.W = dn->width;
  rp.H = dn->height;
  std::memcpy(rp.o, b.o, sizeof rp.o);
  std::memcpy(rp.p00, b.p00, sizeof rp.p00);
  std::memcpy(rp.du, b.du, sizeof rp.du);
  std::memcpy(rp.dv, b.dv, sizeof rp.dv);
  STAGE_HIP_OK(hipSetDevice(dn->device));
  const unsigned blocks = (unsigned)((dn->sizes.pixels + kBlock - 1) / kBlock);
  hipLaunchKernelGGL(srt::denoise::primary_rays_kernel, dim3(blocks), dim3(kBlock), 0, dn->stream, rp);
  STAGE_HIP_OK(hipGetLastError());
  return SRT_OK;
}

int srt_denoise_run(srt_denoiser* dn, const void* accum_rgba32f_dev, int frames, const srt_hit* guide_dev,
                    void* out_rgba32f_dev, void* out_rgba8_dev) {
  return Run(dn, "srt_denoise_run", accum_rgba32f_dev, frames, guide_dev, nullptr, 0.0f, out_rgba32f_dev, out_rgba8_dev);
}

int srt_denoise_run_albedo(srt_denoiser* dn, const void* accum_rgba32f_dev, int frames, const srt_hit* guide_dev,
                           const srt_surface_attr* attrs_dev, float albedo_floor, void* out_rgba32f_dev,
                           void* out_rgba8_dev) {
  if (!srt::surface::ValidFloor(albedo_floor)) {  // before the object is looked at
    srt::SetError("srt_denoise_run_albedo: albedo_floor must be finite and > 0");
    return SRT_ERR_INVALID;
  }
  if (!dn) return SRT_ERR_INVALID;
  if (dn->params.passes == 0) attrs_dev = nullptr;  // ignored: srt_denoise_run's result
  else if (!attrs_dev || !Aligned(attrs_dev, 16)) {
    srt::SetError("srt_denoise_run_albedo: attrs are needed when passes > 0, 16-byte aligned");
    return SRT_ERR_INVALID;
  }
  return Run(dn, "srt_denoise_run_albedo", accum_rgba32f_dev, frames, guide_dev, attrs_dev, albedo_floor, out_rgba32f_dev,
             out_rgba8_dev);
}

int srt_variance_abi_version(void) { return SRT_VARIANCE_ABI_VERSION; }

int srt_denoise_enable_variance(srt_denoiser* dn) {
  if (!dn) return SRT_ERR_INVALID;
  if (dn->d_var[0]) return SRT_OK;
  STAGE_HIP_OK(hipSetDevice(dn->device));
  STAGE_HIP_OK(srt::stage::AllocPair(dn->d_var, srt::denoise::VarianceBytes(dn->sizes)));
  return SRT_OK;
}

int srt_denoise_get_var_params(srt_denoiser* dn, srt_denoise_var_params* p) {
  if (!dn || !p) return SRT_ERR_INVALID;
  *p = dn->var_params;
  return SRT_OK;
}

int srt_denoise_set_var_params(srt_denoiser* dn, const srt_denoise_var_params* p) {
  if (int rc = srt::denoise::ValidateVarParams(p)) {  // before the object is looked at
    srt::SetError("srt_denoise_set_var_params: sigma_lum finite and > 0, min_history 1..65535");
    return rc;
  }
  if (!dn) {
    srt::SetError("srt_denoise_set_var_params: NULL object");
    return SRT_ERR_INVALID;
  }
  dn->var_params = *p;
  return SRT_OK;
}

int srt_denoise_run_variance(srt_denoiser* dn, const void* colour_rgba32f_dev, int frames, const srt_hit* guide_dev,
                             const void* moments_dev, void* out_rgba32f_dev, void* out_rgba8_dev, void* out_var_f32_dev) {
  if (!dn || !colour_rgba32f_dev || !guide_dev || !moments_dev || frames < 1 || (!out_rgba32f_dev && !out_rgba8_dev))
    return SRT_ERR_INVALID;
  if (!dn->d_var[0]) {
    srt::SetError("srt_denoise_run_variance: call srt_denoise_enable_variance first");
    return SRT_ERR_INVALID;
  }
  if (!Aligned(colour_rgba32f_dev, 16) || !Aligned(guide_dev, 16) || !Aligned(moments_dev, 16) ||
      !Aligned(out_rgba32f_dev, 16) || !Aligned(out_rgba8_dev, 4) || !Aligned(out_var_f32_dev, 4)) {
    srt::SetError("srt_denoise_run_variance: colour, guide, moments and out_rgba32f must be 16-byte aligned, out_rgba8 and out_var 4-byte");
    return SRT_ERR_INVALID;
  }
  srt::denoise::VarLaunch sched[SRT_DENOISE_MAX_PASSES + 1];
  const int n = srt::denoise::BuildVarianceSchedule(dn->params, dn->width, dn->height, sched);
  if (n == 0) {
    srt::SetError("srt_denoise_run_variance: passes must be at least 1");
    return SRT_ERR_INVALID;
  }
  STAGE_HIP_OK(hipSetDevice(dn->device));
  srt::denoise::VParams vp;
  std::memset(&vp, 0, sizeof vp);
  vp.hits = reinterpret_cast<const uint4*>(guide_dev);
  vp.moments = static_cast<const float4*>(moments_dev);
  vp.guide = dn->d_guide;
  vp.W = dn->width;
  vp.H = dn->height;
  vp.nsq = (int)dn->params.normal_squarings;
  vp.frames = (float)frames;
  vp.sigma_d = dn->params.sigma_depth;
  vp.sigma_l = dn->var_params.sigma_lum;
  vp.min_history = (float)dn->var_params.min_history;
  for (int i = 0; i < n; ++i) {
    const srt::denoise::VarLaunch& l = sched[i];
    vp.src = l.resolve ? static_cast<const float4*>(colour_rgba32f_dev) : dn->d_color[l.src];
    vp.vsrc = l.resolve ? nullptr : dn->d_var[l.src];
    vp.dst = l.last ? nullptr : dn->d_color[l.dst];
    vp.vdst = l.last ? nullptr : dn->d_var[l.dst];
    vp.out32 = l.last ? static_cast<float4*>(out_rgba32f_dev) : nullptr;
    vp.out8 = l.last ? static_cast<uint32_t*>(out_rgba8_dev) : nullptr;
    vp.outv = l.last ? static_cast<float*>(out_var_f32_dev) : nullptr;
    vp.step = l.step;
    const dim3 grid(l.grid_x, l.grid_y);
    if (l.resolve)
      hipLaunchKernelGGL(srt::denoise::variance_resolve_kernel, grid, dim3(kBlock), 0, dn->stream, vp);
    else
      hipLaunchKernelGGL(srt::denoise::variance_pass_kernel, grid, dim3(kBlock), 0, dn->stream, vp);
    STAGE_HIP_OK(hipGetLastError());
  }
  dn->last_launches = n;
  return SRT_OK;
}

}  // extern "C"
