// tile_cull.hpp -- which 8x8 tiles of a launch can only produce the sky constant: pure host arithmetic, no
// device, no HIP header (pathtrace.hip's Launch reads the answer and deals only the live tiles;
// tests/cpp/test_tile_cull.cpp links tile_cull.cpp alone).
//
// A camera sample whose ray fails the root box test of every BVH record ends at once with
// color = 0 + (1,1,1) * sky (kernels.hpp finish_sample).  A tile is `sky` when that is proved for every
// sample of every frame it can hold, whatever jitter texel the sample draws; accumulate_kernel then
// supplies the constant and sample_kernel never sees the tile.  A false `live` costs only speed, a false
// `sky` changes the image, so every case the argument below does not cover stays `live`.
//
// The argument, per BVH record i < max(bvh_count, 1), in double:
//   * A record whose frame has an all-zero 3x3 linear part maps every direction to 0: every triangle test
//     is then "parallel" and the record never hits (the ghost bvhs[1]; records past
//     the uploaded ones read as zeros and are of this kind).  It is ignored.
//   * Otherwise the tile's samples lie in a pyramid with its apex at the camera centre: pixel columns
//     [8tx - 0.5 + min nz.x, last + 0.5 - 1 + max nz.x] and the global rows its local rows map to, each
//     widened by kCullPixelMargin.  The frame is linear, so the pyramid's four side planes stay planes in the
//     record's frame.  box_t (traversal.hpp) accepts a box *behind* the origin as well (tn <= tf < 0
//     returns tf, which box_ok takes), so the tile must be separated from the rays' whole lines: the root
//     box, expanded by kCullBoxMargin, must lie wholly outside one side plane (no forward ray meets it)
//     and wholly on the inner side of another (no backward ray meets it: the mirrored pyramid lies on
//     the outer side of every plane), each by the plane margin below.
//
// Margins.  With E = 2^-23 (one fp32 ulp, relative):
//   * kCullPixelMargin = 1/64 pixel: (float)x + (nz - 0.5f) rounds to at most 2^-9 pixel at x < 65536.
//   * GetRay's direction: five roundings of terms no larger than S = |center| + |p00| + W|du| + H|dv|
//     (max norms), bounded by 8 E S; through the frame (row sums A) and its own three roundings:
//     A * 16 E S.  Taken kCullSafety = 4 times and divided by the shortest sample direction (bounded below by the
//     distance of the samples' plane from the apex, one value per record) it is the angle
//     the side planes may be off; times the farthest box corner it is the plane margin.
//   * The fp32 slab test is the exact slab test of a box whose planes moved by at most 4 E (|box| + |o|)
//     seen from an origin that is off by 4 E (A |center| + |t|).  kCullBoxMargin = 1e-4 of that scale is
//     over 200 times as much.
// Kept `live` beyond that: a frame, box or camera that is not finite; an apex inside or within the margin
// of the expanded box; a degenerate pyramid (singular frame: no usable side plane); a direction error of
// more than 1% of that shortest direction; scales past 1e30; and the slab test's 0 * inf -- the
// tile's direction interval contains 0 on an axis whose lo or hi plane the origin touches within the
// margin (box_t drops the NaN through fmin / fmax, which no geometric argument covers).
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#include "srt_internal.hpp"

namespace srt {

constexpr double kCullPixelMargin = 1.0 / 64.0;
constexpr double kCullBoxMargin = 1e-4;
constexpr double kCullSafety = 4.0;

struct RootBox {
  float lo[3], hi[3];
};

struct TileCullIn {
  // the launch's camera (pathtrace.hip CameraParams)
  float center[3], p00[3], du[3], dv[3];
  int W = 0, H = 0;            // frame
  int local_rows = 0;          // rows of this rank
  int ext_w = 0, ext_h = 0;    // dispatch extent (global pixels)
  const int* row_map = nullptr;  // global row of each local row; nullptr: the identity (one rank)
  const srt_bvh_record* bvhs = nullptr;  // records [0, n_records); the ones past them read as zeros
  const RootBox* roots = nullptr;        // root box of each record's tree
  size_t n_records = 0;
  uint32_t bvh_count = 0;
  float nz_min[2] = {0, 0}, nz_max[2] = {0, 0};  // exact extremes of noise_xy.x / .y
  bool noise_finite = false;
  bool show_model = false;     // a mesh scene (the sphere scene keeps every tile)
  bool counting = false;       // a counting launch keeps every tile
  bool pool_or_wavefront = false;  // so do pool and wavefront mode
  bool enabled = true;         // SRT_TILE_CULL=0 clears it
};

struct TileCullOut {
  std::vector<uint8_t> sky;    // per local tile (row-major, tiles_x per row): 1 = sky
  int tiles_x = 0, tiles_y = 0;
  int live = 0;                // tiles to trace
  long long culled_pixels = 0; // in-extent pixels of the sky tiles
};

// Global rows [*gmin, *gmax] of local tile row `ty`: its local rows below local_rows, through row_map, that lie
// inside the dispatch extent.  Returns how many there are (0: *gmin > *gmax).  ClassifyTiles takes a tile's
// rows from here.
int TileRowRange(const TileCullIn& in, int ty, int* gmin, int* gmax);

void ClassifyTiles(const TileCullIn& in, TileCullOut* out);

}  // namespace srt
