// tile_cull.cpp -- the conservative sky / live classification of a launch's 8x8 tiles (tile_cull.hpp).
//
// Cost.  A sample's direction in a record's frame is affine in its pixel coordinates, d(u, v) = D0 + Du u + Dv v,
// so the side plane of a tile's pyramid at a column bound u is spanned by D0 + Du u and Dv whatever the tile's
// rows, and the one at a row bound v by D0 + Dv v and Du whatever its columns.  The planes are therefore tested
// once per tile column and once per tile row (two bounds each), and a tile only combines four booleans per
// record: a classification is O(tiles_x + tiles_y) plane tests and O(tiles) byte operations, tens of
// microseconds at 1920x1080, so a camera that moves every frame can afford it.
#include "tile_cull.hpp"

#include <algorithm>
#include <cmath>

namespace srt {

namespace {

constexpr double kE = 1.0 / 8388608.0;  // 2^-23

struct V3 {
  double x, y, z;
};
inline V3 Sub(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
inline V3 Mad(V3 a, V3 b, double s) { return {a.x + b.x * s, a.y + b.y * s, a.z + b.z * s}; }
inline double Dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
inline V3 Cross(V3 a, V3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
inline double Norm(V3 a) { return std::sqrt(Dot(a, a)); }
inline double MaxAbs(V3 a) { return std::max(std::fabs(a.x), std::max(std::fabs(a.y), std::fabs(a.z))); }
inline double Axis(V3 a, int k) { return k == 0 ? a.x : (k == 1 ? a.y : a.z); }
inline V3 F3(const float* f) { return {(double)f[0], (double)f[1], (double)f[2]}; }
inline bool Finite(V3 a) { return std::isfinite(a.x) && std::isfinite(a.y) && std::isfinite(a.z); }

// the frame's linear part applied to v (column-major 4x4, traversal.hpp xform with w = 0)
inline V3 Lin(const float* m, V3 v) {
  return {m[0] * v.x + m[4] * v.y + m[8] * v.z, m[1] * v.x + m[5] * v.y + m[9] * v.z,
          m[2] * v.x + m[6] * v.y + m[10] * v.z};
}

// One record seen from one camera: everything of the test that does not depend on the tile.
struct RecordView {
  bool never_hit = false;  // ignored
  bool usable = false;     // finite, sane scales: tiles may be tested (else every tile is live)
  V3 o{};                  // the apex in the record's frame
  V3 blo{}, bhi{};         // the root box as stored, sorted
  double mb = 0;           // box margin (absolute)
  double derr = 0;         // bound of a sample direction's error in the record's frame (absolute, with kCullSafety)
  double mp = 0;           // plane margin
  double dmax = 0;         // the longest sample direction of the frame
  V3 d0{}, du{}, dv{};     // a sample's direction in the record's frame: d0 + du u + dv v
  V3 rel[8]{};             // the expanded box's corners, from the apex
  bool touch[3] = {false, false, false};  // the origin touches the box's lo or hi plane on this axis (0 * inf)
};

RecordView ViewRecord(const TileCullIn& in, size_t i, double s_world, double u_lo, double u_hi, double v_lo,
                      double v_hi) {
  RecordView r;
  const float* m = in.bvhs[i].frame;
  bool lin_zero = true, fin = true;
  for (int k : {0, 1, 2, 4, 5, 6, 8, 9, 10}) {
    lin_zero = lin_zero && m[k] == 0.0f;
    fin = fin && std::isfinite(m[k]);
  }
  for (int k : {12, 13, 14}) fin = fin && std::isfinite(m[k]);
  if (lin_zero) {  // (whatever its translation: a zero direction is parallel to every triangle)
    r.never_hit = true;
    return r;
  }
  if (!fin) return r;
  const V3 c = F3(in.center), t = {(double)m[12], (double)m[13], (double)m[14]};
  const V3 lc = Lin(m, c);
  r.o = {lc.x + t.x, lc.y + t.y, lc.z + t.z};
  const V3 a = F3(in.roots[i].lo), b = F3(in.roots[i].hi);
  if (!Finite(a) || !Finite(b) || !Finite(r.o)) return r;
  r.blo = {std::min(a.x, b.x), std::min(a.y, b.y), std::min(a.z, b.z)};
  r.bhi = {std::max(a.x, b.x), std::max(a.y, b.y), std::max(a.z, b.z)};
  // row sums of |A|, and the magnitudes the origin's terms reach
  double norm_a = 0, o_scale = 0;
  for (int row = 0; row < 3; ++row) {
    const double ra = std::fabs((double)m[row]) + std::fabs((double)m[4 + row]) + std::fabs((double)m[8 + row]);
    norm_a = std::max(norm_a, ra);
    o_scale = std::max(o_scale, std::fabs((double)m[row] * c.x) + std::fabs((double)m[4 + row] * c.y) +
                                    std::fabs((double)m[8 + row] * c.z) + std::fabs((double)m[12 + row]));
  }
  const double b_scale = std::max(MaxAbs(r.blo), MaxAbs(r.bhi));
  r.mb = kCullBoxMargin * (b_scale + o_scale);
  r.derr = kCullSafety * norm_a * 16.0 * kE * s_world;
  if (!(r.mb < 1e30) || !(r.derr < 1e30)) return r;
  const V3 lo = {r.blo.x - r.mb, r.blo.y - r.mb, r.blo.z - r.mb}, hi = {r.bhi.x + r.mb, r.bhi.y + r.mb, r.bhi.z + r.mb};
  // the apex inside the expanded box, or within the margin of it
  if (r.o.x >= lo.x - r.mb && r.o.x <= hi.x + r.mb && r.o.y >= lo.y - r.mb && r.o.y <= hi.y + r.mb &&
      r.o.z >= lo.z - r.mb && r.o.z <= hi.z + r.mb)
    return r;
  double far = 0;
  for (int k = 0; k < 8; ++k) {
    r.rel[k] = Sub(V3{(k & 1) ? hi.x : lo.x, (k & 2) ? hi.y : lo.y, (k & 4) ? hi.z : lo.z}, r.o);
    far = std::max(far, Norm(r.rel[k]));
  }
  // the samples' directions: affine in the pixel coordinates, all on one plane of the record's frame.  The
  // shortest of them is no shorter than that plane's distance from the apex; the longest is at a corner of
  // the frame (a norm is convex)
  r.d0 = Lin(m, Sub(F3(in.p00), c));
  r.du = Lin(m, F3(in.du));
  r.dv = Lin(m, F3(in.dv));
  if (!Finite(r.d0) || !Finite(r.du) || !Finite(r.dv)) return r;
  const V3 n = Cross(r.du, r.dv);
  const double nn = Norm(n);
  if (!(nn > 0.0) || !std::isfinite(nn)) return r;  // a singular frame: the pyramids are flat
  const double dmin = std::fabs(Dot(r.d0, n)) / nn;
  for (double u : {u_lo, u_hi})
    for (double v : {v_lo, v_hi}) r.dmax = std::max(r.dmax, Norm(Mad(Mad(r.d0, r.du, u), r.dv, v)));
  if (!std::isfinite(r.dmax)) return r;
  if (!(r.derr < 0.01 * dmin)) return r;  // (also an apex on the samples' plane)
  if (!(far < 1e30 * dmin)) return r;     // slab distances far from fp32's overflow
  r.mp = (r.derr / dmin) * far + r.mb;
  for (int k = 0; k < 3; ++k) {
    const double o = Axis(r.o, k);
    r.touch[k] = std::fabs(o - Axis(r.blo, k)) <= 2.0 * r.mb || std::fabs(o - Axis(r.bhi, k)) <= 2.0 * r.mb;
  }
  r.usable = true;
  return r;
}

// What one side plane of a pyramid proves: the box lies wholly beyond it (no forward ray of the pyramid meets
// the box), or wholly on its inner side (no backward ray does).
struct Side {
  bool fwd = false, bwd = false;
};

// The side plane through the apex spanned by `edge` (the samples' direction at the bound, at the other
// coordinate's origin) and `along` (the direction's derivative in the other coordinate).  `across`: its
// derivative in the bound's own coordinate; `inward`: +1 when the pyramid lies at larger values of that
// coordinate (a lower bound), -1 at an upper bound; `width`: the pyramid's extent in it.
Side TestPlane(const RecordView& r, V3 edge, V3 along, V3 across, double inward, double width) {
  Side s;
  V3 n = Cross(edge, along);
  const double nn = Norm(n);
  if (!(nn > 0.0) || !std::isfinite(nn)) return s;
  n = {n.x / nn, n.y / nn, n.z / nn};
  // orientation: the pyramid's opposite edges lie at n . (across * width), strictly on one side (else it is flat here)
  const double side = Dot(n, across) * width;
  if (!(std::fabs(side) > 1e-9 * r.dmax)) return s;
  const double sign = (side > 0.0 ? 1.0 : -1.0) * inward;
  double qmin = 1e300, qmax = -1e300;
  for (int j = 0; j < 8; ++j) {
    const double q = sign * Dot(n, r.rel[j]);
    qmin = std::min(qmin, q);
    qmax = std::max(qmax, q);
  }
  s.fwd = qmax < -r.mp;
  s.bwd = qmin > r.mp;
  return s;
}

// A tile column's or row's share of the test: what its two side planes prove, and its part of the samples'
// direction interval on each axis.
struct Strip {
  bool has = false;      // it holds a sample inside the dispatch extent
  double lo = 0, hi = 0; // its bounds in pixel coordinates (GetRay's ps), margins included
  int pixels = 0;        // its columns / rows inside the extent
};
struct StripView {
  Side side;
  double dmin[3], dmax[3];
};

}  // namespace

int TileRowRange(const TileCullIn& in, int ty, int* gmin, int* gmax) {
  *gmin = 0x7FFFFFFF;
  *gmax = -1;
  int rows = 0;
  for (int ly = ty * 8; ly < ty * 8 + 8 && ly < in.local_rows; ++ly) {
    const int g = in.row_map ? in.row_map[ly] : ly;
    if (g >= in.ext_h) continue;
    *gmin = std::min(*gmin, g);
    *gmax = std::max(*gmax, g);
    ++rows;
  }
  return rows;
}

void ClassifyTiles(const TileCullIn& in, TileCullOut* out) {
  out->tiles_x = (in.W + 7) >> 3;
  out->tiles_y = (in.local_rows + 7) >> 3;
  const int tx_n = std::max(out->tiles_x, 0), ty_n = std::max(out->tiles_y, 0);
  const size_t n = (size_t)tx_n * (size_t)ty_n;
  out->sky.assign(n, 0);
  out->live = (int)n;
  out->culled_pixels = 0;
  if (n == 0 || !in.enabled || !in.show_model || in.counting || in.pool_or_wavefront || !in.noise_finite) return;
  const V3 c = F3(in.center), p00 = F3(in.p00), du = F3(in.du), dv = F3(in.dv);
  if (!Finite(c) || !Finite(p00) || !Finite(du) || !Finite(dv)) return;
  const double s_world = MaxAbs(c) + MaxAbs(p00) + (double)in.W * MaxAbs(du) + (double)in.H * MaxAbs(dv);
  if (!(s_world < 1e30)) return;
  // the tile columns and rows: their pixels inside the extent and their bounds
  std::vector<Strip> cols((size_t)tx_n), rows((size_t)ty_n);
  double u_lo = 0, u_hi = 0, v_lo = 0, v_hi = 0;
  bool any = false;
  for (int tx = 0; tx < tx_n; ++tx) {
    const int x0 = tx * 8, x1 = std::min(std::min(tx * 8 + 7, in.W - 1), in.ext_w - 1);
    Strip& s = cols[(size_t)tx];
    if (x1 < x0) continue;
    s.has = true;
    s.pixels = x1 - x0 + 1;
    s.lo = (double)x0 + ((double)in.nz_min[0] - 0.5) - kCullPixelMargin;
    s.hi = (double)x1 + ((double)in.nz_max[0] - 0.5) + kCullPixelMargin;
    u_lo = any ? std::min(u_lo, s.lo) : s.lo;
    u_hi = any ? std::max(u_hi, s.hi) : s.hi;
    any = true;
  }
  any = false;
  for (int ty = 0; ty < ty_n; ++ty) {
    int gmin = 0, gmax = 0;
    Strip& s = rows[(size_t)ty];
    s.pixels = TileRowRange(in, ty, &gmin, &gmax);
    if (s.pixels == 0) continue;
    s.has = true;
    s.lo = (double)gmin + ((double)in.nz_min[1] - 0.5) - kCullPixelMargin;
    s.hi = (double)gmax + ((double)in.nz_max[1] - 0.5) + kCullPixelMargin;
    v_lo = any ? std::min(v_lo, s.lo) : s.lo;
    v_hi = any ? std::max(v_hi, s.hi) : s.hi;
    any = true;
  }
  // per record that can hit: what each column's and each row's side planes prove
  std::vector<uint8_t> sky(n, 1);
  const size_t records = std::min<size_t>(std::max<size_t>(in.bvh_count, 1), in.n_records);  // (the kernel tests
  // bvhs[0] whatever bvh_count says; the records past the uploaded ones read as zeros and never hit)
  std::vector<StripView> cv((size_t)tx_n), rv((size_t)ty_n);
  for (size_t i = 0; i < records; ++i) {
    const RecordView r = ViewRecord(in, i, s_world, u_lo, u_hi, v_lo, v_hi);
    if (r.never_hit) continue;
    if (!r.usable) return;  // every tile stays live
    const bool touch = r.touch[0] || r.touch[1] || r.touch[2];
    for (int tx = 0; tx < tx_n; ++tx) {
      const Strip& s = cols[(size_t)tx];
      if (!s.has) continue;
      const Side a = TestPlane(r, Mad(r.d0, r.du, s.lo), r.dv, r.du, 1.0, s.hi - s.lo);
      const Side b = TestPlane(r, Mad(r.d0, r.du, s.hi), r.dv, r.du, -1.0, s.hi - s.lo);
      StripView& w = cv[(size_t)tx];
      w.side = Side{a.fwd || b.fwd, a.bwd || b.bwd};
      for (int k = 0; k < 3; ++k) {
        const double p = Axis(r.d0, k) + Axis(r.du, k) * s.lo, q = Axis(r.d0, k) + Axis(r.du, k) * s.hi;
        w.dmin[k] = std::min(p, q);
        w.dmax[k] = std::max(p, q);
      }
    }
    for (int ty = 0; ty < ty_n; ++ty) {
      const Strip& s = rows[(size_t)ty];
      if (!s.has) continue;
      const Side a = TestPlane(r, Mad(r.d0, r.dv, s.lo), r.du, r.dv, 1.0, s.hi - s.lo);
      const Side b = TestPlane(r, Mad(r.d0, r.dv, s.hi), r.du, r.dv, -1.0, s.hi - s.lo);
      StripView& w = rv[(size_t)ty];
      w.side = Side{a.fwd || b.fwd, a.bwd || b.bwd};
      for (int k = 0; k < 3; ++k) {
        const double p = Axis(r.dv, k) * s.lo, q = Axis(r.dv, k) * s.hi;
        w.dmin[k] = std::min(p, q);
        w.dmax[k] = std::max(p, q);
      }
    }
    for (int ty = 0; ty < ty_n; ++ty) {
      if (!rows[(size_t)ty].has) continue;
      const StripView& y = rv[(size_t)ty];
      uint8_t* line = sky.data() + (size_t)ty * (size_t)tx_n;
      for (int tx = 0; tx < tx_n; ++tx) {
        if (!cols[(size_t)tx].has || !line[tx]) continue;
        const StripView& x = cv[(size_t)tx];
        bool ok = (x.side.fwd || y.side.fwd) && (x.side.bwd || y.side.bwd);
        // the slab test's 0 * inf: an axis on which some sample's direction may be 0 while the origin touches
        // one of the box's planes on that axis
        if (ok && touch)
          for (int k = 0; k < 3; ++k)
            if (r.touch[k] && x.dmin[k] + y.dmin[k] - r.derr <= 0.0 && x.dmax[k] + y.dmax[k] + r.derr >= 0.0) ok = false;
        if (!ok) line[tx] = 0;
      }
    }
  }
  for (int ty = 0; ty < ty_n; ++ty)
    for (int tx = 0; tx < tx_n; ++tx) {
      const size_t tile = (size_t)ty * (size_t)tx_n + (size_t)tx;
      // (a tile with no sample inside the extent is sky: nothing to trace, nothing accumulated)
      if (!sky[tile]) continue;
      out->sky[tile] = 1;
      --out->live;
      if (cols[(size_t)tx].has && rows[(size_t)ty].has)
        out->culled_pixels += (long long)cols[(size_t)tx].pixels * rows[(size_t)ty].pixels;
    }
}

}  // namespace srt
