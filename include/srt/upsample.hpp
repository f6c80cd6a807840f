// srt/upsample.hpp -- header-only C++ mirror of include/srt_upsample.h: srt::Upsampler, RAII over the C ABI with
// the same method names.  Errors throw std::runtime_error carrying srt_last_error().
#pragma once

#include <stdexcept>
#include <string>
#include <utility>

#include "../srt_upsample.h"

namespace srt {

class Upsampler {
 public:
  // From low_w x low_h by `factor` (1..4) on `device`; `stream` is a hipStream_t (nullptr: a stream of its own).
  Upsampler(int device, void* stream, int low_w, int low_h, int factor) {
    Check(srt_upsample_create(device, stream, low_w, low_h, factor, &u_), "srt_upsample_create");
  }
  ~Upsampler() {
    if (u_) srt_upsample_destroy(u_);
  }
  Upsampler(const Upsampler&) = delete;
  Upsampler& operator=(const Upsampler&) = delete;
  Upsampler(Upsampler&& o) noexcept : u_(std::exchange(o.u_, nullptr)) {}
  Upsampler& operator=(Upsampler&& o) noexcept {
    if (this != &o) {
      if (u_) srt_upsample_destroy(u_);
      u_ = std::exchange(o.u_, nullptr);
    }
    return *this;
  }

  srt_upsample_params params() const {
    srt_upsample_params p{};
    Check(srt_upsample_get_params(u_, &p), "srt_upsample_get_params");
    return p;
  }
  void set_params(const srt_upsample_params& p) { Check(srt_upsample_set_params(u_, &p), "srt_upsample_set_params"); }
  // Device pointers; only enqueues on the upsampler's stream.
  void run(const void* low_accum_dev, int frames, const srt_hit* low_guide_dev, const srt_hit* full_guide_dev,
           void* out_rgba32f_dev, void* out_rgba8_dev) {
    Check(srt_upsample_run(u_, low_accum_dev, frames, low_guide_dev, full_guide_dev, out_rgba32f_dev, out_rgba8_dev),
          "srt_upsample_run");
  }
  int get_int(const char* name) const {
    int v = 0;
    Check(srt_upsample_get_int(u_, name, &v), name);
    return v;
  }
  void* stream() const { return srt_upsample_stream(u_); }
  srt_upsampler* handle() const { return u_; }

 private:
  static void Check(int rc, const char* what) {
    if (rc != SRT_OK)
      throw std::runtime_error(std::string(what) + " failed with status " + std::to_string(rc) + ": " + srt_last_error());
  }
  srt_upsampler* u_ = nullptr;
};

}  // namespace srt
