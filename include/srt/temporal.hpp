// srt/temporal.hpp -- header-only C++ mirror of include/srt_temporal.h, srt_temporal_motion.h and srt_temporal_deform.h:
// srt::Temporal, RAII over the C ABI with the same method names.  Errors throw std::runtime_error carrying srt_last_error().
#pragma once

#include <stdexcept>
#include <string>
#include <utility>

#include "../srt_temporal.h"
#include "../srt_temporal_deform.h"
#include "../srt_temporal_motion.h"
#include "../srt_variance.h"

namespace srt {

class Temporal {
 public:
  // Full frames of width x height on `device`; `stream` is a hipStream_t (nullptr: a stream of its own).
  Temporal(int device, void* stream, int width, int height) {
    Check(srt_temporal_create(device, stream, width, height, &t_), "srt_temporal_create");
  }
  ~Temporal() {
    if (t_) srt_temporal_destroy(t_);
  }
  Temporal(const Temporal&) = delete;
  Temporal& operator=(const Temporal&) = delete;
  Temporal(Temporal&& o) noexcept : t_(std::exchange(o.t_, nullptr)) {}
  Temporal& operator=(Temporal&& o) noexcept {
    if (this != &o) {
      if (t_) srt_temporal_destroy(t_);
      t_ = std::exchange(o.t_, nullptr);
    }
    return *this;
  }

  srt_temporal_params params() const {
    srt_temporal_params p{};
    Check(srt_temporal_get_params(t_, &p), "srt_temporal_get_params");
    return p;
  }
  void set_params(const srt_temporal_params& p) { Check(srt_temporal_set_params(t_, &p), "srt_temporal_set_params"); }
  // The pose of BVH records 0..n-1 from now on (srt_temporal_motion.h); n == 0: the static behaviour.
  void SetModels(const srt_temporal_model* models, uint32_t n) {
    Check(srt_temporal_set_models(t_, models, n), "srt_temporal_set_models");
  }
  // The mesh whose vertices move (srt_temporal_deform.h): host triangles, read before the call returns; n_tris == 0
  // detaches.  Then, per frame, the DEVICE vertices the frame was traced against (nullptr: every pixel rigid).
  void SetMesh(const srt_triangle* tris, uint32_t n_tris, uint32_t n_verts) {
    Check(srt_temporal_set_mesh(t_, tris, n_tris, n_verts), "srt_temporal_set_mesh");
  }
  void SetVertices(const srt_vertex* verts_dev, uint32_t n_verts) {
    Check(srt_temporal_set_vertices(t_, verts_dev, n_verts), "srt_temporal_set_vertices");
  }
  // world_to_model = frame and its affine inverse.
  static srt_temporal_model ModelFromFrame(const float frame[16]) {
    srt_temporal_model m{};
    Check(srt_temporal_model_from_frame(frame, &m), "srt_temporal_model_from_frame");
    return m;
  }
  // Drops the history (after a scene change, or a model-matrix change that SetModels was not told of).
  void reset() { Check(srt_temporal_reset(t_), "srt_temporal_reset"); }
  // Device pointers; only enqueues on the object's stream.  out receives (colour, N).
  void accumulate(const void* accum_rgba32f_dev, int frames, const srt_hit* guide_dev, const srt_temporal_camera& cam,
                  void* out_rgba32f_dev) {
    Check(srt_temporal_accumulate(t_, accum_rgba32f_dev, frames, guide_dev, &cam, out_rgba32f_dev),
          "srt_temporal_accumulate");
  }
  // Luminance moments (srt_variance.h): allocate their history once, then accumulate with out_moments = (m1, m2, v, N).
  void EnableMoments() { Check(srt_temporal_enable_moments(t_), "srt_temporal_enable_moments"); }
  void AccumulateMoments(const void* accum_rgba32f_dev, int frames, const srt_hit* guide_dev, const srt_temporal_camera& cam,
                         void* out_rgba32f_dev, void* out_moments_dev) {
    Check(srt_temporal_accumulate_moments(t_, accum_rgba32f_dev, frames, guide_dev, &cam, out_rgba32f_dev, out_moments_dev),
          "srt_temporal_accumulate_moments");
  }
  int get_int(const char* name) const {
    int v = 0;
    Check(srt_temporal_get_int(t_, name, &v), name);
    return v;
  }
  void* stream() const { return srt_temporal_stream(t_); }
  srt_temporal* handle() const { return t_; }

 private:
  static void Check(int rc, const char* what) {
    if (rc != SRT_OK)
      throw std::runtime_error(std::string(what) + " failed with status " + std::to_string(rc) + ": " + srt_last_error());
  }
  srt_temporal* t_ = nullptr;
};

}  // namespace srt
