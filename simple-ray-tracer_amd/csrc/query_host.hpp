// query_host.hpp -- host-only parts of the ray-query service (include/srt_query.h): validation of the
// std430 scene arrays, their re-layout for query_kernel and the traversal-stack plan.  No device, no HIP
// header: tests/cpp/test_query_host.cpp links query_host.cpp alone.
#pragma once

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/srt_amd.h"

namespace srt {
namespace query {

struct F4 {
  float x, y, z, w;
};

constexpr uint32_t kTriPad = 1;      // zero records past the triangle array (a leaf step reads two records)
constexpr uint32_t kNoPair = 0xFFFFFFFFu;
constexpr int kBlock = 256;          // lanes per block of query_kernel
constexpr size_t kLdsStackMax = 65536;

// Device layout of a scene.
//   pairs: one 64-B block per sibling pair, (min0 | ref0) (max0 | cnt0) (min1 | ref1) (max1 | cnt1); a
//          leaf's ref is its first triangle and cnt its count, an internal node's ref is the pair index of
//          its children and cnt 0.  Pairs are numbered in the traversal's order (pre-order, right child
//          first); nodes no traversal reaches are dropped.
//   roots: one 32-B record (min | ref) (max | cnt) per BVH record, and record n_bvhs for node 0, where the
//          ghost records past n_bvhs start.
//   tris:  48 B per triangle in input order: v0, e1 = v1 - v0, e2 = v2 - v0, material_idx, index, 0;
//          kTriPad zero records follow.
struct Layout {
  std::vector<F4> pairs, roots, tris;
  uint32_t n_pairs = 0;
  uint32_t max_leaf = 0;  // largest leaf count reached
  int depth = 0;          // deepest node reached (a root has depth 0)
};

// Validates as srt_upload_scene does (every node some traversal reaches, from the BVH records' roots and
// from node 0) and fills `out`.  SRT_OK, or SRT_ERR_INVALID with a message in *err.
int BuildLayout(const srt_bvh_record* bvhs, uint32_t n_bvhs, const srt_bvh_node* nodes, uint32_t n_nodes,
                const srt_triangle* tris, uint32_t n_tris, const srt_vertex* verts, uint32_t n_verts, Layout* out,
                std::string* err);

// Traversal stacks: one entry per tree level and lane (depth + 1 entries).  They live in LDS while a
// block's 3-dword entries fit 64 KiB, otherwise in a per-block lane-interleaved HBM area.  Entries are
// stored in 2 dwords (ref | cnt << 24, t) when every pair and triangle index fits 24 bits and every leaf
// holds fewer than 256 triangles.
struct StackPlan {
  int entries = 1;
  bool in_hbm = false;
  bool packed = false;
  size_t lds_bytes = 0;        // dynamic LDS of a block
  size_t hbm_block_bytes = 0;  // HBM area of a block (0 in LDS mode)
};
StackPlan PlanStack(const Layout& l, uint32_t n_tris);

}  // namespace query
}  // namespace srt
