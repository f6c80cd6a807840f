// srt/denoise.hpp -- header-only C++ mirror of include/srt_denoise.h: srt::Denoiser, RAII over the C ABI with
// the same method names.  Errors throw std::runtime_error carrying srt_last_error().
#pragma once

#include <stdexcept>
#include <string>
#include <utility>

#include "../srt_denoise.h"
#include "../srt_surface.h"
#include "../srt_variance.h"

namespace srt {

// RunAlbedo's default floor (the C ABI has none): chosen on the CPU by tools/albedo_floor_grid.py (DESIGN.md
// section 5, "Surface attributes and demodulation").
constexpr float kAlbedoFloor = 0.1f;

class Denoiser {
 public:
  // Full frames of width x height on `device`; `stream` is a hipStream_t (nullptr: a stream of its own).
  Denoiser(int device, void* stream, int width, int height) {
    Check(srt_denoise_create(device, stream, width, height, &d_), "srt_denoise_create");
  }
  ~Denoiser() {
    if (d_) srt_denoise_destroy(d_);
  }
  Denoiser(const Denoiser&) = delete;
  Denoiser& operator=(const Denoiser&) = delete;
  Denoiser(Denoiser&& o) noexcept : d_(std::exchange(o.d_, nullptr)) {}
  Denoiser& operator=(Denoiser&& o) noexcept {
    if (this != &o) {
      if (d_) srt_denoise_destroy(d_);
      d_ = std::exchange(o.d_, nullptr);
    }
    return *this;
  }

  srt_denoise_params params() const {
    srt_denoise_params p{};
    Check(srt_denoise_get_params(d_, &p), "srt_denoise_get_params");
    return p;
  }
  void set_params(const srt_denoise_params& p) { Check(srt_denoise_set_params(d_, &p), "srt_denoise_set_params"); }
  // Device pointers; both only enqueue on the denoiser's stream.
  void primary_rays(const float origin[3], const float front[3], const float right[3], const float up[3],
                    srt_ray* rays_dev) {
    Check(srt_denoise_primary_rays(d_, origin, front, right, up, rays_dev), "srt_denoise_primary_rays");
  }
  void run(const void* accum_rgba32f_dev, int frames, const srt_hit* guide_dev, void* out_rgba32f_dev,
           void* out_rgba8_dev) {
    Check(srt_denoise_run(d_, accum_rgba32f_dev, frames, guide_dev, out_rgba32f_dev, out_rgba8_dev), "srt_denoise_run");
  }
  // The variance-guided filter (srt_variance.h): allocate the variance arrays once; 1 + passes launches a run.
  void EnableVariance() { Check(srt_denoise_enable_variance(d_), "srt_denoise_enable_variance"); }
  srt_denoise_var_params variance_params() const {
    srt_denoise_var_params p{};
    Check(srt_denoise_get_var_params(d_, &p), "srt_denoise_get_var_params");
    return p;
  }
  void SetVarianceParams(const srt_denoise_var_params& p) {
    Check(srt_denoise_set_var_params(d_, &p), "srt_denoise_set_var_params");
  }
  void RunVariance(const void* colour_rgba32f_dev, int frames, const srt_hit* guide_dev, const void* moments_dev,
                   void* out_rgba32f_dev, void* out_rgba8_dev, void* out_var_f32_dev) {
    Check(srt_denoise_run_variance(d_, colour_rgba32f_dev, frames, guide_dev, moments_dev, out_rgba32f_dev, out_rgba8_dev,
                                   out_var_f32_dev),
          "srt_denoise_run_variance");
  }
  // Albedo-demodulated filtering (srt_surface.h): attrs_dev is Surface::shade's output for the pixel-centre rays.
  void RunAlbedo(const void* accum_rgba32f_dev, int frames, const srt_hit* guide_dev, const srt_surface_attr* attrs_dev,
                 void* out_rgba32f_dev, void* out_rgba8_dev, float albedo_floor = kAlbedoFloor) {
    Check(srt_denoise_run_albedo(d_, accum_rgba32f_dev, frames, guide_dev, attrs_dev, albedo_floor, out_rgba32f_dev,
                                 out_rgba8_dev),
          "srt_denoise_run_albedo");
  }
  int get_int(const char* name) const {
    int v = 0;
    Check(srt_denoise_get_int(d_, name, &v), name);
    return v;
  }
  void* stream() const { return srt_denoise_stream(d_); }
  srt_denoiser* handle() const { return d_; }

 private:
  static void Check(int rc, const char* what) {
    if (rc != SRT_OK)
      throw std::runtime_error(std::string(what) + " failed with status " + std::to_string(rc) + ": " + srt_last_error());
  }
  srt_denoiser* d_ = nullptr;
};

}  // namespace srt
