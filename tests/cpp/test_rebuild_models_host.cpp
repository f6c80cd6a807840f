// The several-model rebuild of include/srt_rebuild_models.h in csrc/rebuild_host.cpp (with csrc/refit_host.cpp, which it
// rests on) as a stand-alone program, meant for AddressSanitizer + UBSan on the CPU (no device, no HIP):
//   g++ -std=c++17 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude
//       tests/cpp/test_rebuild_models_host.cpp simple-ray-tracer_amd/csrc/{rebuild_host,refit_host}.cpp
// (or `make SAN=1 test_rebuild_models_host` in simple-ray-tracer_amd).  The owners from node arrays and from a query
// layout, the segments, the mirror against the single-model mirror run on every record alone -- triangles of the records
// interleaved in the array -- the one-record case byte for byte, the refusals, and the contract functions.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <string>
#include <vector>

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

struct SceneArrays {
  std::vector<srt_bvh_record> bvhs;
  std::vector<srt_bvh_node> nodes;
  std::vector<srt_triangle> tris;
  std::vector<srt_vertex> verts;
  std::vector<uint32_t> owner;  // what the walk must find
};

// `sizes[r]` small triangles per record at random places of a box of the record's own (equal: all at one place), each
// record under a one-triangle-leaf LBVH of its own, blocks concatenated; then the triangle array permuted by `shuffle`
// (the leaves' references follow), so that a record's triangles lie anywhere.
static SceneArrays MakeScene(std::mt19937& rng, const std::vector<int>& sizes, bool equal, bool shuffle) {
  SceneArrays s;
  std::uniform_real_distribution<float> u(0.0f, 16.0f);
  for (size_t r = 0; r < sizes.size(); ++r) {
    const uint32_t tri_base = (uint32_t)s.tris.size(), node_base = (uint32_t)s.nodes.size();
    for (int t = 0; t < sizes[r]; ++t) {
      const float x = 40.0f * r + (equal ? 1.0f : u(rng)), y = equal ? 2.0f : u(rng), z = equal ? 3.0f : u(rng);
      const float p[3][3] = {{x, y, z}, {x + 0.25f, y, z + 0.125f}, {x, y + 0.25f, z}};
      const uint32_t v0 = (uint32_t)s.verts.size();
      for (int c = 0; c < 3; ++c) {
        srt_vertex v{};
        for (int a = 0; a < 3; ++a) v.vertex[a] = p[c][a];
        s.verts.push_back(v);
      }
      s.tris.push_back(srt_triangle{v0, v0 + 1, v0 + 2, (uint32_t)(100 * r + t)});
      s.owner.push_back((uint32_t)r);
    }
    const uint32_t n = (uint32_t)sizes[r];
    std::vector<srt_bvh_node> nodes(2 * n - 1);
    std::vector<srt_triangle> sorted(n);
    std::vector<uint32_t> order(n);
    std::string err;
    CHECK(BuildLBVH(s.tris.data() + tri_base, n, s.verts.data(), (uint32_t)s.verts.size(), nodes.data(), sorted.data(),
                    order.data(), &err) == SRT_OK);
    std::copy(sorted.begin(), sorted.end(), s.tris.begin() + tri_base);
    for (srt_bvh_node& nd : nodes) {
      nd.first_child_or_prim_index += nd.prim_count ? tri_base : node_base;
      s.nodes.push_back(nd);
    }
    srt_bvh_record rec{};
    rec.first_index = node_base;
    rec.count = 2 * n - 1;
    rec.frame[0] = rec.frame[5] = rec.frame[10] = rec.frame[15] = 1.0f + r;
    s.bvhs.push_back(rec);
  }
  if (shuffle) {
    const uint32_t n = (uint32_t)s.tris.size();
    std::vector<uint32_t> to(n);
    for (uint32_t t = 0; t < n; ++t) to[t] = t;
    std::shuffle(to.begin(), to.end(), rng);
    std::vector<srt_triangle> tris(n);
    std::vector<uint32_t> owner(n);
    for (uint32_t t = 0; t < n; ++t) {
      tris[to[t]] = s.tris[t];
      owner[to[t]] = s.owner[t];
    }
    s.tris = tris;
    s.owner = owner;
    for (srt_bvh_node& nd : s.nodes)
      if (nd.prim_count) nd.first_child_or_prim_index = to[nd.first_child_or_prim_index];
  }
  return s;
}

struct Built {
  int rc = 0;
  std::string err;
  std::vector<srt_bvh_record> bvhs;
  std::vector<srt_bvh_node> nodes;
  std::vector<srt_triangle> tris;
  std::vector<uint32_t> order;
};

static Built Build(const SceneArrays& s, uint32_t max_leaf) {
  const uint32_t n = (uint32_t)s.tris.size();
  Built b;
  b.bvhs.resize(s.bvhs.size());
  b.nodes.resize(2 * (size_t)n - 1);
  b.tris.resize(n);
  b.order.assign(n, 77u);
  uint32_t n_nodes = 0;
  b.rc = BuildLBVHModels(s.bvhs.data(), (uint32_t)s.bvhs.size(), s.nodes.data(), (uint32_t)s.nodes.size(), s.tris.data(), n,
                         s.verts.data(), (uint32_t)s.verts.size(), max_leaf, b.bvhs.data(), b.nodes.data(), &n_nodes,
                         b.tris.data(), b.order.data(), &b.err);
  b.nodes.resize(b.rc ? 0 : n_nodes);
  return b;
}

// The mirror against the single-model mirror on every record alone.
static void CheckAgainstRecords(const SceneArrays& s, uint32_t max_leaf) {
  const Built b = Build(s, max_leaf);
  CHECK(b.rc == SRT_OK);
  if (b.rc) return;
  const uint32_t n = (uint32_t)s.tris.size();
  size_t node_at = 0;
  uint32_t pos = 0;
  for (uint32_t r = 0; r < s.bvhs.size(); ++r) {
    std::vector<uint32_t> mine;
    std::vector<srt_triangle> tris;
    for (uint32_t t = 0; t < n; ++t)
      if (s.owner[t] == r) {
        mine.push_back(t);
        tris.push_back(s.tris[t]);
      }
    const uint32_t c = (uint32_t)mine.size();
    std::vector<srt_bvh_node> nodes(2 * c - 1);
    std::vector<srt_triangle> sorted(c);
    std::vector<uint32_t> order(c);
    uint32_t n_nodes = 0;
    std::string err;
    CHECK(BuildLBVHLeaf(tris.data(), c, s.verts.data(), (uint32_t)s.verts.size(), max_leaf, nodes.data(), &n_nodes,
                        sorted.data(), order.data(), &err) == SRT_OK);
    CHECK(b.bvhs[r].first_index == node_at && b.bvhs[r].count == s.bvhs[r].count);
    CHECK(std::memcmp(b.bvhs[r].frame, s.bvhs[r].frame, sizeof b.bvhs[r].frame) == 0);
    CHECK(node_at + n_nodes <= b.nodes.size());
    if (node_at + n_nodes > b.nodes.size()) return;
    for (uint32_t j = 0; j < n_nodes; ++j) {
      srt_bvh_node want = nodes[j];
      want.first_child_or_prim_index += want.prim_count ? pos : (uint32_t)node_at;
      CHECK(std::memcmp(&want, &b.nodes[node_at + j], sizeof want) == 0);
    }
    for (uint32_t p = 0; p < c; ++p) {
      CHECK(b.order[pos + p] == mine[order[p]]);
      CHECK(std::memcmp(&b.tris[pos + p], &sorted[p], sizeof(srt_triangle)) == 0);
    }
    node_at += n_nodes;
    pos += c;
  }
  CHECK(node_at == b.nodes.size() && pos == n);
}

static void CheckOwners() {
  std::mt19937 rng(5);
  for (bool shuffle : {false, true}) {
    const SceneArrays s = MakeScene(rng, {9, 1, 3, 17}, false, shuffle);
    const uint32_t n = (uint32_t)s.tris.size();
    std::vector<uint32_t> owner(n, 5u);
    std::string err;
    CHECK(OwnersFromNodes(s.bvhs.data(), 4, s.nodes.data(), (uint32_t)s.nodes.size(), n, owner.data(), &err) == SRT_OK);
    CHECK(owner == s.owner);
    const Segments seg = SegmentsOf(owner.data(), n, 4);
    CHECK((seg.count == std::vector<uint32_t>{9, 1, 3, 17}) && (seg.first == std::vector<uint32_t>{0, 9, 10, 13}));
    uint32_t pairs = 0, leaf = 0;
    SegmentShape(seg, 1, &pairs, &leaf);
    CHECK(pairs == 8 + 2 + 16 && leaf == 1);
    SegmentShape(seg, 4, &pairs, &leaf);
    CHECK(pairs == 8 + 16 && leaf == 3);
    SegmentShape(seg, 255, &pairs, &leaf);
    CHECK(pairs == 0 && leaf == 17);
    CHECK(CheckSegments(seg, &err) == SRT_OK);
    Segments hole = seg;
    hole.count[1] = 0;
    CHECK(CheckSegments(hole, &err) == SRT_ERR_INVALID && err.find("must own at least one triangle") != std::string::npos);
  }
  // a query layout by hand: record 0's root is pair 0 = (leaf 0, pair 1), pair 1 = (leaf 3 x2, leaf 2); record 1's root
  // is the leaf (1, 1); the ghost root repeats record 0's
  using srt::query::F4;
  auto w = [](uint32_t u) {
    float f;
    std::memcpy(&f, &u, 4);
    return f;
  };
  auto rec = [&](uint32_t ref, uint32_t cnt, F4* at) {
    at[0] = F4{0, 0, 0, w(ref)};
    at[1] = F4{0, 0, 0, w(cnt)};
  };
  std::vector<F4> pairs(8), roots(6);
  rec(0, 1, &pairs[0]);
  rec(1, 0, &pairs[2]);
  rec(3, 2, &pairs[4]);
  rec(2, 1, &pairs[6]);
  rec(0, 0, &roots[0]);
  rec(1, 1, &roots[2]);
  rec(0, 0, &roots[4]);
  std::vector<uint32_t> owner(5, 9u);
  std::string err;
  CHECK(OwnersFromLayout(pairs.data(), 2, roots.data(), 2, 5, owner.data(), &err) == SRT_OK);
  CHECK((owner == std::vector<uint32_t>{0, 1, 0, 0, 0}));
  // an orphan (a sixth triangle), a triangle of two records, a shared pair, references out of range
  std::vector<uint32_t> six(6);
  CHECK(OwnersFromLayout(pairs.data(), 2, roots.data(), 2, 6, six.data(), &err) == SRT_ERR_INVALID);
  CHECK(err.find("exactly one BVH record") != std::string::npos);
  rec(2, 1, &roots[2]);
  CHECK(OwnersFromLayout(pairs.data(), 2, roots.data(), 2, 5, owner.data(), &err) == SRT_ERR_INVALID);
  CHECK(err.find("exactly one BVH record") != std::string::npos);
  rec(1, 0, &roots[2]);
  CHECK(OwnersFromLayout(pairs.data(), 2, roots.data(), 2, 5, owner.data(), &err) == SRT_ERR_INVALID);
  CHECK(err.find("exactly one BVH record") != std::string::npos);
  rec(2, 0, &roots[2]);
  CHECK(OwnersFromLayout(pairs.data(), 2, roots.data(), 2, 5, owner.data(), &err) == SRT_ERR_INVALID);
  rec(4, 2, &roots[2]);
  CHECK(OwnersFromLayout(pairs.data(), 2, roots.data(), 2, 5, owner.data(), &err) == SRT_ERR_INVALID);
  rec(1, 0, &pairs[2]);
  rec(0, 0, &pairs[6]);  // a cycle inside record 0
  rec(1, 1, &roots[2]);
  CHECK(OwnersFromLayout(pairs.data(), 2, roots.data(), 2, 5, owner.data(), &err) == SRT_ERR_INVALID);
}

static void CheckRefusals() {
  std::mt19937 rng(9);
  const SceneArrays good = MakeScene(rng, {6, 4}, false, false);
  CHECK(Build(good, 1).rc == SRT_OK);
  {  // record 1 shares record 0's root
    SceneArrays s = good;
    s.bvhs[1].first_index = 0;
    const Built b = Build(s, 1);
    CHECK(b.rc == SRT_ERR_INVALID && b.err.find("exactly one BVH record") != std::string::npos);
    CHECK(std::all_of(b.order.begin(), b.order.end(), [](uint32_t o) { return o == 77u; }));
  }
  {  // a leaf of record 1 names a triangle of record 0
    SceneArrays s = good;
    for (size_t j = s.bvhs[1].first_index; j < s.nodes.size(); ++j)
      if (s.nodes[j].prim_count) {
        s.nodes[j].first_child_or_prim_index = 0;
        break;
      }
    const Built b = Build(s, 4);
    CHECK(b.rc == SRT_ERR_INVALID && b.err.find("exactly one BVH record") != std::string::npos);
  }
  {  // an orphan: one more triangle than the trees reach
    SceneArrays s = good;
    s.tris.push_back(s.tris[0]);
    const Built b = Build(s, 1);
    CHECK(b.rc == SRT_ERR_INVALID && b.err.find("exactly one BVH record") != std::string::npos);
  }
  {  // record 0 does not start at node 0
    SceneArrays s = good;
    std::swap(s.bvhs[0], s.bvhs[1]);
    const Built b = Build(s, 1);
    CHECK(b.rc == SRT_ERR_INVALID && b.err.find("first_index") != std::string::npos);
  }
  {  // the single-model mirror's refusals
    CHECK(Build(good, 0).rc == SRT_ERR_INVALID && Build(good, 256).rc == SRT_ERR_INVALID);
    CHECK(Build(good, 0).err.find("[1, 255]") != std::string::npos);
    SceneArrays s = good;
    s.verts[2].vertex[1] = std::numeric_limits<float>::infinity();
    const Built b = Build(s, 1);
    CHECK(b.rc == SRT_ERR_INVALID && b.err.find("not finite") != std::string::npos);
    s = good;
    s.nodes[1].first_child_or_prim_index = 1u << 20;
    CHECK(Build(s, 1).rc == SRT_ERR_INVALID);
    std::string err;
    uint32_t nn = 0, o = 0;
    srt_bvh_record rec{};
    srt_bvh_node nd{};
    srt_triangle tr{};
    CHECK(BuildLBVHModels(nullptr, 1, &nd, 1, &tr, 1, good.verts.data(), 3, 1, &rec, &nd, &nn, &tr, &o, &err) == SRT_ERR_INVALID);
    CHECK(BuildLBVHModels(&rec, 1, &nd, 1, &tr, 0, good.verts.data(), 3, 1, &rec, &nd, &nn, &tr, &o, &err) == SRT_ERR_INVALID);
    CHECK(err.find("srt_bvh_build_lbvh_models: a tree needs at least one triangle") != std::string::npos);
    CHECK(BuildLBVHModels(&rec, 0, &nd, 1, &tr, 1, good.verts.data(), 3, 1, &rec, &nd, &nn, &tr, &o, &err) == SRT_ERR_INVALID);
    CHECK(BuildLBVHModels(&rec, 1, &nd, 1, &tr, 1u << 30, good.verts.data(), 3, 1, &rec, &nd, &nn, &tr, &o, &err) == SRT_ERR_LIMIT);
  }
}

static void CheckContract() {
  std::string err;
  CHECK(CheckEnableModels(true, true, 0, 100, &err) == SRT_OK);
  CHECK(CheckEnableModels(false, true, 0, 100, &err) == SRT_ERR_INVALID && err.find("null object") != std::string::npos);
  CHECK(CheckEnableModels(true, false, 0, 100, &err) == SRT_ERR_INVALID && err.find("SRT_QUERY_REFIT") != std::string::npos);
  CHECK(CheckEnableModels(true, true, 3, 100, &err) == SRT_ERR_INVALID && err.find("first_index") != std::string::npos);
  CHECK(CheckEnableModels(true, true, 0, 1u << 30, &err) == SRT_ERR_LIMIT);
  // the old call keeps its refusal
  CHECK(CheckEnable(true, true, 2, 0, 100, &err) == SRT_ERR_INVALID && err.find("more than one BVH record") != std::string::npos);
  CHECK(ModelsSummaryValid(0, 0, 0, 4) && ModelsSummaryValid(3, 4, 10, 4) && ModelsSummaryValid(10, 1, 10, 4));
  CHECK(!ModelsSummaryValid(0, 0, 10, 4) && !ModelsSummaryValid(11, 2, 10, 4) && !ModelsSummaryValid(3, 5, 10, 4));
  CHECK(!ModelsSummaryValid(3, 0, 10, 4) && !ModelsSummaryValid(1, 1, 0, 4));
}

int main() {
  std::mt19937 rng(1);
  for (uint32_t max_leaf : {1u, 2u, 4u, 255u}) {
    for (bool shuffle : {false, true}) {
      CheckAgainstRecords(MakeScene(rng, {40, 7}, false, shuffle), max_leaf);
      CheckAgainstRecords(MakeScene(rng, {16, 1, 3}, true, shuffle), max_leaf);  // ties: local positions decide
      CheckAgainstRecords(MakeScene(rng, {1, 1}, false, shuffle), max_leaf);
      CheckAgainstRecords(MakeScene(rng, {2, 5, 1, 33}, false, shuffle), max_leaf);
    }
    // one record: srt_bvh_build_lbvh_leaf byte for byte (CheckAgainstRecords with pos == node_at == 0)
    CheckAgainstRecords(MakeScene(rng, {29}, false, false), max_leaf);
  }
  CheckOwners();
  CheckRefusals();
  CheckContract();
  if (g_fail) {
    std::fprintf(stderr, "%d checks failed\n", g_fail);
    return 1;
  }
  std::printf("rebuild models host checks OK\n");
  return 0;
}
