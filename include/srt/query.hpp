// srt/query.hpp -- header-only C++ mirror of include/srt_query.h: srt::Query, RAII over the C ABI with the
// same method names.  Errors throw std::runtime_error carrying srt_last_error().
#pragma once

#include <cstdint>
#include <stdexcept>
#include <string>
#include <utility>

#include "../srt_query.h"

namespace srt {

class Query {
 public:
  // The std430 arrays srt_upload_scene takes; `stream` is a hipStream_t (nullptr: a stream of its own).
  Query(int device, void* stream, const srt_bvh_record* bvhs, uint32_t n_bvhs, const srt_bvh_node* nodes,
        uint32_t n_nodes, const srt_triangle* tris, uint32_t n_tris, const srt_vertex* verts, uint32_t n_verts) {
    Check(srt_query_create(device, stream, bvhs, n_bvhs, nodes, n_nodes, tris, n_tris, verts, n_verts, &q_),
          "srt_query_create");
  }
  Query(int device, void* stream, const srt_scene* scene) {
    Check(srt_query_create_obj(device, stream, scene, &q_), "srt_query_create_obj");
  }
  ~Query() {
    if (q_) srt_query_destroy(q_);
  }
  Query(const Query&) = delete;
  Query& operator=(const Query&) = delete;
  Query(Query&& o) noexcept : q_(std::exchange(o.q_, nullptr)) {}
  Query& operator=(Query&& o) noexcept {
    if (this != &o) {
      if (q_) srt_query_destroy(q_);
      q_ = std::exchange(o.q_, nullptr);
    }
    return *this;
  }

  void set_bvh_count(uint32_t n) { Check(srt_query_set_bvh_count(q_, n), "srt_query_set_bvh_count"); }
  void update_model_matrix(uint32_t index, const float frame[16]) {
    Check(srt_query_update_model_matrix(q_, index, frame), "srt_query_update_model_matrix");
  }
  // Device pointers; both only enqueue on the query's stream.
  void closest(const srt_ray* rays_dev, uint32_t n, srt_hit* hits_dev) {
    Check(srt_query_closest(q_, rays_dev, n, hits_dev), "srt_query_closest");
  }
  void occluded(const srt_ray* rays_dev, uint32_t n, uint8_t* occluded_dev) {
    Check(srt_query_occluded(q_, rays_dev, n, occluded_dev), "srt_query_occluded");
  }
  int get_int(const char* name) const {
    int v = 0;
    Check(srt_query_get_int(q_, name, &v), name);
    return v;
  }
  void* stream() const { return srt_query_stream(q_); }
  srt_query* handle() const { return q_; }

 private:
  static void Check(int rc, const char* what) {
    if (rc != SRT_OK)
      throw std::runtime_error(std::string(what) + " failed with status " + std::to_string(rc) + ": " + srt_last_error());
  }
  srt_query* q_ = nullptr;
};

}  // namespace srt
