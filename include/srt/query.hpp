// srt/query.hpp -- header-only C++ mirror of include/srt_query.h, include/srt_refit.h, include/srt_rebuild.h,
// include/srt_rebuild_leaf.h, include/srt_rebuild_models.h and include/srt_query_sort.h: srt::Query, RAII over the C ABI
// with the same method names, AssetUtils::RefitBVH, AssetUtils::BuildLBVH, AssetUtils::BuildLBVHModels and
// AssetUtils::RayOrder.
// Errors throw std::runtime_error carrying srt_last_error().
#pragma once

#include <cstdint>
#include <stdexcept>
#include <string>
#include <utility>

#include "../srt_query.h"
#include "../srt_query_sort.h"
#include "../srt_rebuild.h"
#include "../srt_rebuild_leaf.h"
#include "../srt_rebuild_models.h"
#include "../srt_refit.h"

namespace srt {

class Query {
 public:
  // The std430 arrays srt_upload_scene takes; `stream` is a hipStream_t (nullptr: a stream of its own);
  // `flags`: 0, or SRT_QUERY_REFIT for an object Refit() can move to new vertices.
  Query(int device, void* stream, const srt_bvh_record* bvhs, uint32_t n_bvhs, const srt_bvh_node* nodes,
        uint32_t n_nodes, const srt_triangle* tris, uint32_t n_tris, const srt_vertex* verts, uint32_t n_verts,
        uint32_t flags = 0) {
    Check(srt_query_create_ex(device, stream, bvhs, n_bvhs, nodes, n_nodes, tris, n_tris, verts, n_verts, flags, &q_),
          "srt_query_create_ex");
  }
  Query(int device, void* stream, const srt_scene* scene, uint32_t flags = 0) {
    Check(srt_query_create_obj_ex(device, stream, scene, flags, &q_), "srt_query_create_obj_ex");
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
  // srt_query_refit: `verts_dev` is a device array of `n` srt_vertex records; only enqueues on the query's stream.
  void Refit(const srt_vertex* verts_dev, uint32_t n) { Check(srt_query_refit(q_, verts_dev, n), "srt_query_refit"); }
  // include/srt_rebuild.h, for an object created with SRT_QUERY_REFIT over one model: EnableRebuild allocates, Rebuild
  // builds a linear BVH over the triangles at `verts_dev` on the device (it synchronises the stream once).
  void EnableRebuild() { Check(srt_query_enable_rebuild(q_), "srt_query_enable_rebuild"); }
  void Rebuild(const srt_vertex* verts_dev, uint32_t n) { Check(srt_query_rebuild(q_, verts_dev, n), "srt_query_rebuild"); }
  // include/srt_rebuild_leaf.h: from the next Rebuild on, subtrees of at most `max_leaf` triangles (1..255) are leaves.
  void SetRebuildLeaf(uint32_t max_leaf) { Check(srt_query_set_rebuild_leaf(q_, max_leaf), "srt_query_set_rebuild_leaf"); }
  // include/srt_rebuild_models.h: EnableRebuild for a scene of any number of BVH records; Rebuild then gives every record
  // the tree of its own triangles.
  void EnableRebuildModels() { Check(srt_query_enable_rebuild_models(q_), "srt_query_enable_rebuild_models"); }
  // Device pointers; both only enqueue on the query's stream.
  void closest(const srt_ray* rays_dev, uint32_t n, srt_hit* hits_dev) {
    Check(srt_query_closest(q_, rays_dev, n, hits_dev), "srt_query_closest");
  }
  void occluded(const srt_ray* rays_dev, uint32_t n, uint8_t* occluded_dev) {
    Check(srt_query_occluded(q_, rays_dev, n, occluded_dev), "srt_query_occluded");
  }
  // include/srt_query_sort.h: the same calls through a coherence-sorted order built on the device; the same results.
  void ClosestSorted(const srt_ray* rays_dev, uint32_t n, srt_hit* hits_dev) {
    Check(srt_query_closest_sorted(q_, rays_dev, n, hits_dev), "srt_query_closest_sorted");
  }
  void OccludedSorted(const srt_ray* rays_dev, uint32_t n, uint8_t* occluded_dev) {
    Check(srt_query_occluded_sorted(q_, rays_dev, n, occluded_dev), "srt_query_occluded_sorted");
  }
  // The last sorted call's permutation and sorted keys (host arrays of n; nullptr skips); synchronises.
  void CopyRayOrder(uint32_t* order, uint32_t* keys, uint32_t n) {
    Check(srt_query_copy_ray_order(q_, order, keys, n), "srt_query_copy_ray_order");
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

namespace AssetUtils {

// srt_bvh_refit: the bounds of every reached node of `nodes`, in place, refit to `verts` (the topology stays).
inline void RefitBVH(const srt_bvh_record* bvhs, uint32_t n_bvhs, srt_bvh_node* nodes, uint32_t n_nodes,
                     const srt_triangle* tris, uint32_t n_tris, const srt_vertex* verts, uint32_t n_verts) {
  if (int rc = srt_bvh_refit(bvhs, n_bvhs, nodes, n_nodes, tris, n_tris, verts, n_verts))
    throw std::runtime_error("srt_bvh_refit failed with status " + std::to_string(rc) + ": " + srt_last_error());
}

// srt_bvh_build_lbvh: the host mirror of Query::Rebuild -- 2 * n_tris - 1 nodes (root node 0), the triangles in the
// tree's order and position -> input index.
inline void BuildLBVH(const srt_triangle* tris, uint32_t n_tris, const srt_vertex* verts, uint32_t n_verts,
                      srt_bvh_node* nodes_out, srt_triangle* tris_out, uint32_t* order_out) {
  if (int rc = srt_bvh_build_lbvh(tris, n_tris, verts, n_verts, nodes_out, tris_out, order_out))
    throw std::runtime_error("srt_bvh_build_lbvh failed with status " + std::to_string(rc) + ": " + srt_last_error());
}

// srt_bvh_build_lbvh_leaf: the same with subtrees of at most `max_leaf` triangles collapsed into leaves; returns the
// number of nodes written (2m + 1; nodes_out has room for 2 * n_tris - 1).
inline uint32_t BuildLBVH(const srt_triangle* tris, uint32_t n_tris, const srt_vertex* verts, uint32_t n_verts, uint32_t max_leaf,
                          srt_bvh_node* nodes_out, srt_triangle* tris_out, uint32_t* order_out) {
  uint32_t n_nodes = 0;
  if (int rc = srt_bvh_build_lbvh_leaf(tris, n_tris, verts, n_verts, max_leaf, nodes_out, &n_nodes, tris_out, order_out))
    throw std::runtime_error("srt_bvh_build_lbvh_leaf failed with status " + std::to_string(rc) + ": " + srt_last_error());
  return n_nodes;
}

// srt_bvh_build_lbvh_models: the host mirror of Query::Rebuild after EnableRebuildModels -- a block of nodes per BVH
// record in record order (bvhs_out[r].first_index is its start), triangles and order sorted by (record, key); returns the
// number of nodes written (nodes_out has room for 2 * n_tris - 1).
inline uint32_t BuildLBVHModels(const srt_bvh_record* bvhs, uint32_t n_bvhs, const srt_bvh_node* nodes, uint32_t n_nodes,
                                const srt_triangle* tris, uint32_t n_tris, const srt_vertex* verts, uint32_t n_verts,
                                uint32_t max_leaf, srt_bvh_record* bvhs_out, srt_bvh_node* nodes_out, srt_triangle* tris_out,
                                uint32_t* order_out) {
  uint32_t n_out = 0;
  if (int rc = srt_bvh_build_lbvh_models(bvhs, n_bvhs, nodes, n_nodes, tris, n_tris, verts, n_verts, max_leaf, bvhs_out,
                                         nodes_out, &n_out, tris_out, order_out))
    throw std::runtime_error("srt_bvh_build_lbvh_models failed with status " + std::to_string(rc) + ": " + srt_last_error());
  return n_out;
}

// srt_ray_order: the host mirror of Query::ClosestSorted's ordering -- order[n], the stable sort of 0 .. n-1 by key;
// keys[n] (sorted) and bounds[6] (lo xyz, hi xyz of the finite origins) may be nullptr.
inline void RayOrder(const srt_ray* rays, uint32_t n, uint32_t* order, uint32_t* keys = nullptr, float* bounds = nullptr) {
  if (int rc = srt_ray_order(rays, n, order, keys, bounds))
    throw std::runtime_error("srt_ray_order failed with status " + std::to_string(rc) + ": " + srt_last_error());
}

}  // namespace AssetUtils

}  // namespace srt
