// The host-only parts of the device rebuild (csrc/rebuild_host.cpp, with csrc/refit_host.cpp and csrc/query_host.cpp
// it rests on) as a stand-alone program, meant for AddressSanitizer + UBSan on the CPU (no device, no HIP):
//   g++ -std=c++17 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude
//       tests/cpp/test_rebuild_host.cpp simple-ray-tracer_amd/csrc/{rebuild_host,refit_host,query_host}.cpp
// (or `make SAN=1 test_rebuild_host` in simple-ray-tracer_amd).  The key and the prefix at their edges, Karras' node
// against a scan of the prefix rule, the built tree (a permutation, one triangle a leaf, accepted by BuildLayout, boxes
// a fixed point of the refit, depth under its bound), the degenerate sizes, the argument contract of the object calls,
// and the schedule from per-height counts against BuildSchedule.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <string>
#include <vector>

#include "../../simple-ray-tracer_amd/csrc/query_host.hpp"
#include "../../simple-ray-tracer_amd/csrc/rebuild_host.hpp"

using namespace srt::rebuild;

static int g_fail = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
      ++g_fail;                                                            \
    }                                                                      \
  } while (0)

static srt_vertex V(float x, float y, float z) {
  srt_vertex v{};
  v.vertex[0] = x;
  v.vertex[1] = y;
  v.vertex[2] = z;
  return v;
}

static void TestKey() {
  const float inf = std::numeric_limits<float>::infinity();
  CHECK(Cell(0.0f, 0.0f, 0.0f, 0.0f) == 0u);             // no extent
  CHECK(Cell(2.0f, 2.0f, 2.0f, 2.0f) == 0u);
  CHECK(Cell(0.0f, 1.0f, 0.0f, 0.0f) == 0u);
  CHECK(Cell(0.0f, 1.0f, 1.0f, 1.0f) == 1023u);           // u == 1024 clamps
  CHECK(Cell(0.0f, 1024.0f, 5.0f, 6.0f) == 5u);           // c = 5.5
  CHECK(Cell(0.0f, 1024.0f, 1023.0f, 1023.0f) == 1023u);
  CHECK(Cell(-4.0f, 4.0f, -0.0f, 0.0f) == 512u);
  CHECK(Cell(-3e38f, 3e38f, 1.0f, 2.0f) == 0u);           // ext overflows to inf: r == 0
  CHECK(Cell(0.0f, 1.0f, 3e38f, 3e38f) == 1023u);         // c overflows to +inf
  CHECK(Cell(0.0f, 1.0f, -3e38f, -3e38f) == 0u);          // and to -inf
  CHECK(Cell(-inf, inf, 0.0f, 0.0f) == 0u);               // a NaN quotient
  CHECK(Morton(1023, 0, 0) == 0x24924924u && Morton(0, 1023, 0) == 0x12492492u && Morton(0, 0, 1023) == 0x09249249u);
  CHECK(Morton(512, 0, 0) == (1u << 29) && Morton(0, 0, 1) == 1u && Morton(1023, 1023, 1023) == 0x3FFFFFFFu);
}

// The split of [first, last] by the rule's words alone: after the last position whose prefix with `first` is longer
// than the range's own.
static int64_t ScanSplit(const std::vector<uint32_t>& k, int64_t first, int64_t last) {
  const int64_t n = (int64_t)k.size();
  const int own = Prefix(k.data(), n, first, last);
  int64_t g = first;
  for (int64_t x = first; x < last; ++x)
    if (Prefix(k.data(), n, first, x) > own) g = x;
  return g;
}

static void CheckHierarchy(const std::vector<uint32_t>& k) {
  const int64_t n = (int64_t)k.size();
  struct Range {
    int64_t node, first, last;
  };
  std::vector<Range> st{{0, 0, n - 1}};
  int64_t seen = 0;
  while (!st.empty()) {
    const Range r = st.back();
    st.pop_back();
    ++seen;
    Child l, rt;
    KarrasNode(k.data(), n, r.node, &l, &rt);
    const int64_t g = ScanSplit(k, r.first, r.last);
    CHECK(l.index == (uint32_t)g && rt.index == (uint32_t)g + 1);
    CHECK(l.leaf == (r.first == g) && rt.leaf == (r.last == g + 1));
    if (l.index != (uint32_t)g || rt.index != (uint32_t)g + 1) return;
    if (!l.leaf) st.push_back({g, r.first, g});
    if (!rt.leaf) st.push_back({g + 1, g + 1, r.last});
  }
  CHECK(seen == n - 1);  // every internal node is some range's
}

static void TestHierarchy() {
  std::vector<uint32_t> two{3, 9};
  CHECK(Prefix(two.data(), 2, 0, 1) == 28 && Prefix(two.data(), 2, 0, -1) == -1 && Prefix(two.data(), 2, 1, 2) == -1);
  std::vector<uint32_t> same{7, 7, 7, 7};
  CHECK(Prefix(same.data(), 4, 0, 1) == 32 + 31 && Prefix(same.data(), 4, 0, 2) == 32 + 30 && Prefix(same.data(), 4, 1, 2) == 32 + 30);
  Child l, r;
  KarrasNode(two.data(), 2, 0, &l, &r);
  CHECK(l.leaf && r.leaf && l.index == 0 && r.index == 1);
  CheckHierarchy(two);
  CheckHierarchy({5, 5});
  CheckHierarchy({1, 2, 3});
  CheckHierarchy(std::vector<uint32_t>(64, 0x2AAAAAAAu));  // every key equal: the positions decide
  CheckHierarchy(std::vector<uint32_t>(37, 0u));
  std::mt19937 rng(12345);
  for (int round = 0; round < 40; ++round) {
    const int n = 2 + (int)(rng() % 300);
    std::vector<uint32_t> k(n);
    const uint32_t mask = round % 3 == 0 ? 0x3FFFFFFFu : (round % 3 == 1 ? 0x1Fu : 0x30000003u);  // many duplicates too
    for (auto& x : k) x = rng() & mask;
    std::sort(k.begin(), k.end());
    CheckHierarchy(k);
  }
}

struct Mesh {
  std::vector<srt_triangle> tris;
  std::vector<srt_vertex> verts;
};

static Mesh RandomMesh(uint32_t n_tris, uint32_t seed, bool flat) {
  std::mt19937 rng(seed);
  std::uniform_real_distribution<float> u(-4.0f, 9.0f), d(-0.6f, 0.6f);
  Mesh m;
  for (uint32_t t = 0; t < n_tris; ++t) {
    const float c[3] = {u(rng), u(rng), flat ? 2.0f : u(rng)};
    for (int k = 0; k < 3; ++k) m.verts.push_back(V(c[0] + d(rng), c[1] + d(rng), flat ? 2.0f : c[2] + d(rng)));
    m.tris.push_back(srt_triangle{3 * t, 3 * t + 1, 3 * t + 2, t % 5});
  }
  return m;
}

struct Built {
  std::vector<srt_bvh_node> nodes;
  std::vector<srt_triangle> tris;
  std::vector<uint32_t> order;
  int rc = 0;
  std::string err;
};

static Built Build(const Mesh& m) {
  Built b;
  const uint32_t n = (uint32_t)m.tris.size();
  b.nodes.assign(n ? 2 * (size_t)n - 1 : 1, srt_bvh_node{});
  b.tris.assign(n ? n : 1, srt_triangle{});
  b.order.assign(n ? n : 1, 0xFFFFFFFFu);
  b.rc = BuildLBVH(m.tris.data(), n, m.verts.data(), (uint32_t)m.verts.size(), b.nodes.data(), b.tris.data(), b.order.data(),
                   &b.err);
  return b;
}

static void CheckBuilt(const Mesh& m) {
  const uint32_t n = (uint32_t)m.tris.size();
  Built b = Build(m);
  CHECK(b.rc == SRT_OK);
  if (b.rc != SRT_OK) return;
  // the order: a permutation, sorted by key, ties in input order; the triangles follow it
  std::vector<uint32_t> keys(n);
  Keys(m.tris.data(), n, m.verts.data(), (uint32_t)m.verts.size(), keys.data());
  std::vector<uint8_t> seen(n, 0);
  for (uint32_t p = 0; p < n; ++p) {
    CHECK(b.order[p] < n && !seen[b.order[p]]);
    if (b.order[p] >= n) return;
    seen[b.order[p]] = 1;
    CHECK(std::memcmp(&b.tris[p], &m.tris[b.order[p]], sizeof(srt_triangle)) == 0);
    if (p) CHECK(keys[b.order[p - 1]] < keys[b.order[p]] || (keys[b.order[p - 1]] == keys[b.order[p]] && b.order[p - 1] < b.order[p]));
  }
  // the host validation of srt_query_create accepts the tree; every leaf holds one triangle and every triangle a leaf
  srt_bvh_record rec{};
  srt::query::Layout lay;
  std::string err;
  CHECK(srt::query::BuildLayout(&rec, 1, b.nodes.data(), (uint32_t)b.nodes.size(), b.tris.data(), n, m.verts.data(),
                                (uint32_t)m.verts.size(), &lay, &err) == SRT_OK);
  CHECK(lay.n_pairs == n - 1 && lay.max_leaf == 1);
  CHECK(lay.depth <= DepthBound(n) && lay.depth + 1 <= 64);
  const srt::query::StackPlan plan = srt::query::PlanStack(lay, n);
  CHECK(plan.packed && plan.entries == lay.depth + 1);
  std::vector<uint32_t> leaves(n, 0);
  for (const srt_bvh_node& nd : b.nodes)
    if (nd.prim_count) {
      CHECK(nd.prim_count == 1 && nd.first_child_or_prim_index < n);
      if (nd.first_child_or_prim_index < n) ++leaves[nd.first_child_or_prim_index];
    }
  for (uint32_t c : leaves) CHECK(c == 1);
  // the boxes are the refit's: refitting the built nodes changes no bit
  auto again = b.nodes;
  CHECK(srt::refit::RefitNodes(&rec, 1, again.data(), (uint32_t)again.size(), b.tris.data(), n, m.verts.data(),
                               (uint32_t)m.verts.size(), &err) == SRT_OK);
  CHECK(std::memcmp(again.data(), b.nodes.data(), again.size() * sizeof(srt_bvh_node)) == 0);
  // the schedule the rebuild derives from per-height counts is BuildSchedule's
  const srt::refit::Schedule want = srt::refit::BuildSchedule(lay);
  uint32_t counts[kHeightBins] = {};
  for (uint32_t h = 0; h < want.heights; ++h) counts[h] = want.first[h + 1] - want.first[h];
  srt::refit::Schedule got;
  CHECK(ScheduleFromCounts(counts, kHeightBins, lay.n_pairs, &got));
  CHECK(got.heights == want.heights && got.tail_begin == want.tail_begin && got.launches == want.launches && got.first == want.first);
  CHECK((int)want.heights == lay.depth);  // what the rebuild plans the stack from
  if (want.heights) {
    counts[0] += 1;
    CHECK(!ScheduleFromCounts(counts, kHeightBins, lay.n_pairs, &got));  // pairs that do not add up
  }
}

static void TestBuild() {
  for (uint32_t n : {1u, 2u, 3u, 4u, 5u, 17u, 64u, 257u, 1000u}) {
    CheckBuilt(RandomMesh(n, 100 + n, false));
    CheckBuilt(RandomMesh(n, 200 + n, true));  // flat: one axis without extent
  }
  // 64 copies of one triangle: every key equal, the tree is balanced over the positions
  Mesh copies;
  for (uint32_t t = 0; t < 64; ++t) {
    copies.verts.push_back(V(0.5f, 0.25f, 1.0f));
    copies.verts.push_back(V(2.5f, 0.75f, 1.5f));
    copies.verts.push_back(V(1.0f, 3.0f, -0.5f));
    copies.tris.push_back(srt_triangle{3 * t, 3 * t + 1, 3 * t + 2, 0});
  }
  CheckBuilt(copies);
  Built b = Build(copies);
  for (uint32_t p = 0; p < 64; ++p) CHECK(b.order[p] == p);
  // an index past n_verts reads (0, 0, 0) and widens the scene box
  Mesh oob = RandomMesh(20, 7, false);
  for (auto& v : oob.verts) v.vertex[0] += 20.0f;
  oob.tris[3].v1_idx = 0xFFFFFFF0u;
  oob.tris[9].v0_idx = (uint32_t)oob.verts.size();
  CheckBuilt(oob);
  b = Build(oob);
  CHECK(b.nodes[0].min_bounds[0] == 0.0f);
  // sizes 1 and 2
  b = Build(RandomMesh(1, 3, false));
  CHECK(b.nodes.size() == 1 && b.nodes[0].prim_count == 1 && b.nodes[0].first_child_or_prim_index == 0 && b.order[0] == 0);
  b = Build(RandomMesh(2, 4, false));
  CHECK(b.nodes[0].prim_count == 0 && b.nodes[0].first_child_or_prim_index == 1 && b.nodes[1].prim_count == 1 &&
        b.nodes[2].prim_count == 1 && b.nodes[1].first_child_or_prim_index == 0 && b.nodes[2].first_child_or_prim_index == 1);
  // rejected, with the outputs untouched
  Mesh bad = RandomMesh(6, 5, false);
  for (float v : {std::numeric_limits<float>::infinity(), -std::numeric_limits<float>::infinity(), std::numeric_limits<float>::quiet_NaN()}) {
    const float keep = bad.verts[4].vertex[2];
    bad.verts[4].vertex[2] = v;
    b = Build(bad);
    CHECK(b.rc == SRT_ERR_INVALID && b.err.find("not finite") != std::string::npos && b.order[0] == 0xFFFFFFFFu);
    bad.verts[4].vertex[2] = keep;
  }
  b = Build(Mesh{});
  CHECK(b.rc == SRT_ERR_INVALID);
  std::string err;
  srt_bvh_node nd{};
  srt_triangle tr{};
  uint32_t ord = 0;
  CHECK(BuildLBVH(nullptr, 1, bad.verts.data(), 18, &nd, &tr, &ord, &err) == SRT_ERR_INVALID);
  CHECK(BuildLBVH(bad.tris.data(), 1, nullptr, 18, &nd, &tr, &ord, &err) == SRT_ERR_INVALID);
  CHECK(BuildLBVH(bad.tris.data(), 1, bad.verts.data(), 18, nullptr, &tr, &ord, &err) == SRT_ERR_INVALID);
  CHECK(BuildLBVH(bad.tris.data(), 1, bad.verts.data(), 18, &nd, nullptr, &ord, &err) == SRT_ERR_INVALID);
  CHECK(BuildLBVH(bad.tris.data(), 1, bad.verts.data(), 18, &nd, &tr, nullptr, &err) == SRT_ERR_INVALID);
  CHECK(BuildLBVH(bad.tris.data(), 1u << 30, bad.verts.data(), 18, &nd, &tr, &ord, &err) == SRT_ERR_LIMIT);
  CHECK(DepthBound(1) == 30 && DepthBound(2) == 31 && DepthBound(3) == 32 && DepthBound(1188) == 41 && DepthBound((1u << 30) - 1) == 60);
}

static void TestContract() {
  std::string err;
  alignas(16) static char buf[64];
  CHECK(CheckEnable(false, false, 0, 0, 0, &err) == SRT_ERR_INVALID && err.find("null object") != std::string::npos);
  CHECK(CheckEnable(true, false, 1, 0, 10, &err) == SRT_ERR_INVALID && err.find("without SRT_QUERY_REFIT") != std::string::npos);
  CHECK(CheckEnable(true, true, 2, 0, 10, &err) == SRT_ERR_INVALID && err.find("more than one BVH record") != std::string::npos);
  CHECK(CheckEnable(true, true, 1, 4, 10, &err) == SRT_ERR_INVALID && err.find("first_index") != std::string::npos);
  CHECK(CheckEnable(true, true, 1, 0, 1u << 30, &err) == SRT_ERR_LIMIT);
  CHECK(CheckEnable(true, true, 1, 0, 10, &err) == SRT_OK);
  CHECK(CheckRebuild(false, false, false, buf, 3, 3, &err) == SRT_ERR_INVALID && err.find("null object") != std::string::npos);
  CHECK(CheckRebuild(true, false, false, buf, 3, 3, &err) == SRT_ERR_INVALID && err.find("without SRT_QUERY_REFIT") != std::string::npos);
  CHECK(CheckRebuild(true, true, false, buf, 3, 3, &err) == SRT_ERR_INVALID && err.find("not enabled") != std::string::npos);
  CHECK(CheckRebuild(true, true, true, nullptr, 3, 3, &err) == SRT_ERR_INVALID && err.find("16-byte aligned") != std::string::npos);
  CHECK(CheckRebuild(true, true, true, buf + 4, 3, 3, &err) == SRT_ERR_INVALID && err.find("16-byte aligned") != std::string::npos);
  CHECK(CheckRebuild(true, true, true, buf, 4, 3, &err) == SRT_ERR_INVALID && err.find("n_verts differs") != std::string::npos);
  CHECK(CheckRebuild(true, true, true, buf, 3, 3, &err) == SRT_OK);
}

int main() {
  TestKey();
  TestHierarchy();
  TestBuild();
  TestContract();
  if (g_fail) {
    std::fprintf(stderr, "%d check(s) failed\n", g_fail);
    return 1;
  }
  std::printf("rebuild host checks OK\n");
  return 0;
}
