// srt/surface.hpp -- header-only C++ mirror of include/srt_surface.h and srt_surface_refit.h: srt::Surface, RAII over the C ABI with the
// same method names.  Errors throw std::runtime_error carrying srt_last_error().  (srt_denoise_run_albedo is
// srt::Denoiser::RunAlbedo in srt/denoise.hpp.)
#pragma once

#include <cstdint>
#include <stdexcept>
#include <string>
#include <utility>

#include "../srt_surface.h"
#include "../srt_surface_refit.h"

namespace srt {

class Surface {
 public:
  // The std430 arrays srt_upload_scene takes; `stream` is a hipStream_t (nullptr: a stream of its own).
  Surface(int device, void* stream, const srt_bvh_record* bvhs, uint32_t n_bvhs, const srt_material_obj* mats,
          const float* tex_albedo, uint32_t n_mats, const srt_triangle* tris, uint32_t n_tris, const srt_vertex* verts,
          uint32_t n_verts) {
    Check(srt_surface_create(device, stream, bvhs, n_bvhs, mats, tex_albedo, n_mats, tris, n_tris, verts, n_verts, &s_),
          "srt_surface_create");
  }
  Surface(int device, void* stream, const srt_scene* scene) {
    Check(srt_surface_create_obj(device, stream, scene, &s_), "srt_surface_create_obj");
  }
  // With flags (srt_surface_refit.h): SRT_SURFACE_REFIT makes Refit possible; 0 is the constructors above.
  Surface(int device, void* stream, const srt_bvh_record* bvhs, uint32_t n_bvhs, const srt_material_obj* mats,
          const float* tex_albedo, uint32_t n_mats, const srt_triangle* tris, uint32_t n_tris, const srt_vertex* verts,
          uint32_t n_verts, uint32_t flags) {
    Check(srt_surface_create_ex(device, stream, bvhs, n_bvhs, mats, tex_albedo, n_mats, tris, n_tris, verts, n_verts, flags, &s_),
          "srt_surface_create_ex");
  }
  Surface(int device, void* stream, const srt_scene* scene, uint32_t flags) {
    Check(srt_surface_create_obj_ex(device, stream, scene, flags, &s_), "srt_surface_create_obj_ex");
  }
  ~Surface() {
    if (s_) srt_surface_destroy(s_);
  }
  Surface(const Surface&) = delete;
  Surface& operator=(const Surface&) = delete;
  Surface(Surface&& o) noexcept : s_(std::exchange(o.s_, nullptr)) {}
  Surface& operator=(Surface&& o) noexcept {
    if (this != &o) {
      if (s_) srt_surface_destroy(s_);
      s_ = std::exchange(o.s_, nullptr);
    }
    return *this;
  }

  void upload_textures(const srt_texture* textures, uint32_t n) {
    Check(srt_surface_upload_textures(s_, textures, n), "srt_surface_upload_textures");
  }
  void update_model_matrix(uint32_t index, const float frame[16]) {
    Check(srt_surface_update_model_matrix(s_, index, frame), "srt_surface_update_model_matrix");
  }
  void set_bvh_count(uint32_t n) { Check(srt_surface_set_bvh_count(s_, n), "srt_surface_set_bvh_count"); }
  // Moves the triangles to the DEVICE vertices srt_query_refit was given; only enqueues one launch.
  void Refit(const srt_vertex* verts_dev, uint32_t n_verts) { Check(srt_surface_refit(s_, verts_dev, n_verts), "srt_surface_refit"); }
  // Device pointers; only enqueues one launch on the object's stream.
  void shade(const srt_ray* rays_dev, const srt_hit* hits_dev, uint32_t n, srt_surface_attr* attrs_dev) {
    Check(srt_surface_shade(s_, rays_dev, hits_dev, n, attrs_dev), "srt_surface_shade");
  }
  int get_int(const char* name) const {
    int v = 0;
    Check(srt_surface_get_int(s_, name, &v), name);
    return v;
  }
  void* stream() const { return srt_surface_stream(s_); }
  srt_surface* handle() const { return s_; }

 private:
  static void Check(int rc, const char* what) {
    if (rc != SRT_OK)
      throw std::runtime_error(std::string(what) + " failed with status " + std::to_string(rc) + ": " + srt_last_error());
  }
  srt_surface* s_ = nullptr;
};

}  // namespace srt
