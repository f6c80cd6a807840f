// rebuild_host.cpp -- see rebuild_host.hpp.
#include "rebuild_host.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <numeric>

namespace srt {
namespace rebuild {

namespace {

int Fail(std::string* err, const char* msg, int rc = SRT_ERR_INVALID) {
  if (err) *err = msg;
  return rc;
}

float Vert(const srt_vertex* verts, uint32_t n_verts, uint32_t i, int k) { return i < n_verts ? verts[i].vertex[k] : 0.0f; }

// min / max over a triangle's three vertices, one component; only the values matter (rule 1)
void Span(const srt_triangle& t, const srt_vertex* verts, uint32_t n_verts, int k, float* mn, float* mx) {
  const float a = Vert(verts, n_verts, t.v0_idx, k), b = Vert(verts, n_verts, t.v1_idx, k), c = Vert(verts, n_verts, t.v2_idx, k);
  *mn = refit::FoldMin(refit::FoldMin(a, b), c);
  *mx = refit::FoldMax(refit::FoldMax(a, b), c);
}

// Rule 2: the key of a triangle in the box [lo, hi] of its record
uint32_t Key(const srt_triangle& t, const srt_vertex* verts, uint32_t n_verts, const float* lo, const float* hi) {
  uint32_t q[3];
  for (int k = 0; k < 3; ++k) {
    float mn, mx;
    Span(t, verts, n_verts, k, &mn, &mx);
    q[k] = Cell(lo[k], hi[k], mn, mx);
  }
  return Morton(q[0], q[1], q[2]);
}

// Rule 3: the stable order of the input indices by key (a Morton key, or a (record, key)), the triangles and the order
// out; returns the sorted keys' low dwords, which rule 4 reads.
template <class K>
std::vector<uint32_t> SortByKey(const std::vector<K>& keys, const srt_triangle* tris, srt_triangle* tris_out, uint32_t* order_out) {
  const uint32_t n = (uint32_t)keys.size();
  std::vector<uint32_t> order(n), sorted(n);
  std::iota(order.begin(), order.end(), 0u);
  std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return keys[a] < keys[b]; });
  for (uint32_t p = 0; p < n; ++p) {
    sorted[p] = (uint32_t)keys[order[p]];
    tris_out[p] = tris[order[p]];
    order_out[p] = order[p];
  }
  return sorted;
}

// Rule 4 with 4a-4c over the segment [s, s + c) of the sorted keys (c >= 1), a block of nodes from `base`: the block's
// root, then -- every node's split, the survivors' ranks by increasing index -- the children of the k-th survivor at block
// nodes 2k + 1 and 2k + 2.  With max_leaf == 1 every internal node survives and its rank is its local index.  Returns the
// block's node count, 2m + 1.
size_t PutSegment(const uint32_t* sorted, uint32_t s, uint32_t c, uint32_t max_leaf, size_t base, srt_bvh_node* nodes_out) {
  std::vector<Split> split;
  std::vector<uint32_t> rank;
  auto put = [&](size_t at, const Slot& slot) {
    nodes_out[at] = srt_bvh_node{};
    nodes_out[at].first_child_or_prim_index = slot.count ? slot.index : (uint32_t)(base + 2 * (size_t)rank[slot.index - s] + 1);
    nodes_out[at].prim_count = slot.count;
  };
  const Slot root = SegmentRoot(s, c, max_leaf);
  uint32_t m = 0;
  if (root.count == 0) {
    split.resize(c - 1);
    rank.resize(c - 1);
    for (uint32_t k = 0; k + 1 < c; ++k) {
      split[k] = SegmentSplit(sorted, s, c, s + k);
      rank[k] = m;
      if (Survives(split[k], max_leaf)) ++m;
    }
  }
  put(base, root);
  for (uint32_t k = 0; k < split.size(); ++k) {
    if (!Survives(split[k], max_leaf)) continue;
    put(base + 2 * (size_t)rank[k] + 1, LeftSlot(split[k], max_leaf));
    put(base + 2 * (size_t)rank[k] + 2, RightSlot(split[k], max_leaf));
  }
  return 2 * (size_t)m + 1;
}

}  // namespace

void SceneBox(const srt_triangle* tris, uint32_t n_tris, const srt_vertex* verts, uint32_t n_verts, float lo[3], float hi[3]) {
  for (int k = 0; k < 3; ++k) {
    Span(tris[0], verts, n_verts, k, &lo[k], &hi[k]);
    for (uint32_t t = 1; t < n_tris; ++t) {
      float mn, mx;
      Span(tris[t], verts, n_verts, k, &mn, &mx);
      lo[k] = refit::FoldMin(lo[k], mn);
      hi[k] = refit::FoldMax(hi[k], mx);
    }
  }
}

void Keys(const srt_triangle* tris, uint32_t n_tris, const srt_vertex* verts, uint32_t n_verts, uint32_t* keys) {
  float lo[3], hi[3];
  SceneBox(tris, n_tris, verts, n_verts, lo, hi);
  for (uint32_t t = 0; t < n_tris; ++t) keys[t] = Key(tris[t], verts, n_verts, lo, hi);
}

int DepthBound(uint32_t n_tris) {
  int log2 = 0;
  while (log2 < 32 && (1ull << log2) < n_tris) ++log2;
  return 30 + log2;
}

int BuildLBVH(const srt_triangle* tris, uint32_t n_tris, const srt_vertex* verts, uint32_t n_verts, srt_bvh_node* nodes_out,
              srt_triangle* tris_out, uint32_t* order_out, std::string* err) {
  uint32_t n_nodes = 0;  // 2 * n_tris - 1: every internal node survives
  return BuildLBVHLeaf(tris, n_tris, verts, n_verts, 1, nodes_out, &n_nodes, tris_out, order_out, err);
}

int BuildLBVHLeaf(const srt_triangle* tris, uint32_t n_tris, const srt_vertex* verts, uint32_t n_verts, uint32_t max_leaf,
                  srt_bvh_node* nodes_out, uint32_t* n_nodes_out, srt_triangle* tris_out, uint32_t* order_out, std::string* err) {
  if (!tris || !nodes_out || !n_nodes_out || !tris_out || !order_out || (n_verts && !verts)) return Fail(err, "null argument");
  if (max_leaf == 0 || max_leaf > kMaxLeafLimit) return Fail(err, "srt_bvh_build_lbvh_leaf: max_leaf must be in [1, 255]");
  if (n_tris == 0) return Fail(err, "srt_bvh_build_lbvh: a tree needs at least one triangle");
  if (n_tris >= kMaxTris) return Fail(err, "srt_bvh_build_lbvh: 2^30 triangles or more", SRT_ERR_LIMIT);
  for (uint32_t i = 0; i < n_verts; ++i)
    for (int k = 0; k < 3; ++k)
      if (!std::isfinite(verts[i].vertex[k])) return Fail(err, "srt_bvh_build_lbvh: a vertex position is not finite");
  // rules 1-3: keys in the scene box, in input order, then the stable order; rule 4: one segment, its block at node 0
  std::vector<uint32_t> keys(n_tris);
  Keys(tris, n_tris, verts, n_verts, keys.data());
  const std::vector<uint32_t> sorted = SortByKey(keys, tris, tris_out, order_out);
  const size_t n_nodes = PutSegment(sorted.data(), 0, n_tris, max_leaf, 0, nodes_out);
  *n_nodes_out = (uint32_t)n_nodes;
  // rule 5: srt_refit.h's fold on the new topology (which also walks the tree: a malformed one fails here)
  srt_bvh_record rec{};
  return refit::RefitNodes(&rec, 1, nodes_out, (uint32_t)n_nodes, tris_out, n_tris, verts, n_verts, err);
}

int CheckEnable(bool have_object, bool refit, uint32_t n_bvhs, uint32_t first_index, uint32_t n_tris, std::string* err) {
  if (!have_object) return Fail(err, "srt_query_enable_rebuild: null object");
  if (!refit) return Fail(err, "srt_query_enable_rebuild: the object was created without SRT_QUERY_REFIT");
  if (n_bvhs != 1) return Fail(err, "srt_query_enable_rebuild: the scene has more than one BVH record (one model is the scope)");
  if (first_index != 0) return Fail(err, "srt_query_enable_rebuild: the BVH record's first_index is not 0");
  if (n_tris >= kMaxTris) return Fail(err, "srt_query_enable_rebuild: 2^30 triangles or more", SRT_ERR_LIMIT);
  return SRT_OK;
}

int CheckRebuild(bool have_object, bool refit, bool enabled, const void* verts_dev, uint32_t n_verts, uint32_t want_verts,
                 std::string* err) {
  if (!have_object) return Fail(err, "srt_query_rebuild: null object");
  if (!refit) return Fail(err, "srt_query_rebuild: the object was created without SRT_QUERY_REFIT");
  if (!enabled) return Fail(err, "srt_query_rebuild: rebuild is not enabled (srt_query_enable_rebuild)");
  if (!verts_dev || (reinterpret_cast<uintptr_t>(verts_dev) & 15u))
    return Fail(err, "srt_query_rebuild: verts_dev must be a 16-byte aligned device pointer");
  if (n_verts != want_verts) return Fail(err, "srt_query_rebuild: n_verts differs from the count at creation");
  return SRT_OK;
}

int CheckSetLeaf(bool have_object, bool enabled, uint32_t max_leaf, std::string* err) {
  if (!have_object) return Fail(err, "srt_query_set_rebuild_leaf: null object");
  if (!enabled) return Fail(err, "srt_query_set_rebuild_leaf: rebuild is not enabled (srt_query_enable_rebuild)");
  if (max_leaf == 0 || max_leaf > kMaxLeafLimit) return Fail(err, "srt_query_set_rebuild_leaf: max_leaf must be in [1, 255]");
  return SRT_OK;
}

// -- include/srt_rebuild_models.h -----------------------------------------------------------------------------------------
namespace {

constexpr uint32_t kNoRecord = 0xFFFFFFFFu;
const char* const kOwnership = "every triangle must belong to exactly one BVH record";
const char* const kEmptyRecord = "every BVH record must own at least one triangle";

uint32_t AsUint(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  return u;
}

// One reference met on a walk: a leaf's triangles get their owner; an internal reference is pushed once.
struct OwnerWalk {
  uint32_t n_tris;
  uint32_t* owner;
  std::vector<uint32_t> reached;  // per node or pair: the record that reached it
  std::vector<uint32_t> stack;
  const char* where;

  int Leaf(uint32_t record, uint32_t first, uint32_t count, std::string* err) {
    if ((uint64_t)first + count > n_tris) return Fail(err, "BVH leaf references triangles out of range");
    for (uint32_t t = first; t < first + count; ++t) {
      if (owner[t] != kNoRecord) return Fail(err, (std::string(where) + ": " + kOwnership + " (one has two)").c_str());
      owner[t] = record;
    }
    return SRT_OK;
  }
  int Internal(uint32_t record, uint32_t ref, std::string* err) {
    if (ref >= reached.size()) return Fail(err, "BVH internal node references children out of range (or a cycle)");
    if (reached[ref] != kNoRecord) {
      if (reached[ref] != record) return Fail(err, (std::string(where) + ": " + kOwnership + " (records share nodes)").c_str());
      return Fail(err, "BVH internal node references children out of range (or a cycle)");
    }
    reached[ref] = record;
    stack.push_back(ref);
    return SRT_OK;
  }
  int Finish(std::string* err) {
    for (uint32_t t = 0; t < n_tris; ++t)
      if (owner[t] == kNoRecord) return Fail(err, (std::string(where) + ": " + kOwnership + " (one has none)").c_str());
    return SRT_OK;
  }
};

}  // namespace

int OwnersFromNodes(const srt_bvh_record* bvhs, uint32_t n_bvhs, const srt_bvh_node* nodes, uint32_t n_nodes, uint32_t n_tris,
                    uint32_t* owner, std::string* err) {
  OwnerWalk w{n_tris, owner, std::vector<uint32_t>(n_nodes, kNoRecord), {}, "srt_bvh_build_lbvh_models"};
  std::fill(owner, owner + n_tris, kNoRecord);
  for (uint32_t r = 0; r < n_bvhs; ++r) {
    if (bvhs[r].first_index >= n_nodes) return Fail(err, "BVH first_index out of range");
    // (a root is a reference like any other: a root two records name is a shared node)
    const srt_bvh_node& root = nodes[bvhs[r].first_index];
    if (root.prim_count > 0) {
      if (int rc = w.Leaf(r, root.first_child_or_prim_index, root.prim_count, err)) return rc;
      continue;
    }
    if (int rc = w.Internal(r, bvhs[r].first_index, err)) return rc;
    while (!w.stack.empty()) {
      const uint32_t c = nodes[w.stack.back()].first_child_or_prim_index;
      w.stack.pop_back();
      if ((uint64_t)c + 1 >= n_nodes) return Fail(err, "BVH internal node references children out of range (or a cycle)");
      for (uint32_t k = 0; k < 2; ++k) {
        const srt_bvh_node& n = nodes[c + k];
        const int rc = n.prim_count > 0 ? w.Leaf(r, n.first_child_or_prim_index, n.prim_count, err) : w.Internal(r, c + k, err);
        if (rc) return rc;
      }
    }
  }
  return w.Finish(err);
}

int OwnersFromLayout(const query::F4* pairs, uint32_t n_pairs, const query::F4* roots, uint32_t n_bvhs, uint32_t n_tris,
                     uint32_t* owner, std::string* err) {
  OwnerWalk w{n_tris, owner, std::vector<uint32_t>(n_pairs, kNoRecord), {}, "srt_query_enable_rebuild_models"};
  std::fill(owner, owner + n_tris, kNoRecord);
  auto slot = [&](uint32_t r, const query::F4* rec) {
    const uint32_t ref = AsUint(rec[0].w), cnt = AsUint(rec[1].w);
    return cnt > 0 ? w.Leaf(r, ref, cnt, err) : w.Internal(r, ref, err);
  };
  for (uint32_t r = 0; r < n_bvhs; ++r) {
    if (int rc = slot(r, roots + 2 * (size_t)r)) return rc;
    while (!w.stack.empty()) {
      const query::F4* p = pairs + 4 * (size_t)w.stack.back();
      w.stack.pop_back();
      if (int rc = slot(r, p)) return rc;
      if (int rc = slot(r, p + 2)) return rc;
    }
  }
  return w.Finish(err);
}

Segments SegmentsOf(const uint32_t* owner, uint32_t n_tris, uint32_t n_bvhs) {
  Segments seg;
  seg.first.assign(n_bvhs, 0);
  seg.count.assign(n_bvhs, 0);
  for (uint32_t t = 0; t < n_tris; ++t)
    if (owner[t] < n_bvhs) ++seg.count[owner[t]];
  for (uint32_t r = 1; r < n_bvhs; ++r) seg.first[r] = seg.first[r - 1] + seg.count[r - 1];
  return seg;
}

int CheckSegments(const Segments& seg, std::string* err) {
  for (uint32_t c : seg.count)
    if (c == 0) return Fail(err, kEmptyRecord);
  return SRT_OK;
}

void SegmentShape(const Segments& seg, uint32_t max_leaf, uint32_t* karras_pairs, uint32_t* largest_root_leaf) {
  *karras_pairs = 0;
  *largest_root_leaf = 0;
  for (uint32_t c : seg.count) {
    if (c > max_leaf) *karras_pairs += c - 1;
    else if (c > *largest_root_leaf) *largest_root_leaf = c;
  }
}

int BuildLBVHModels(const srt_bvh_record* bvhs, uint32_t n_bvhs, const srt_bvh_node* nodes, uint32_t n_nodes,
                    const srt_triangle* tris, uint32_t n_tris, const srt_vertex* verts, uint32_t n_verts, uint32_t max_leaf,
                    srt_bvh_record* bvhs_out, srt_bvh_node* nodes_out, uint32_t* n_nodes_out, srt_triangle* tris_out,
                    uint32_t* order_out, std::string* err) {
  if (!bvhs || !nodes || !tris || !bvhs_out || !nodes_out || !n_nodes_out || !tris_out || !order_out || (n_verts && !verts))
    return Fail(err, "null argument");
  if (max_leaf == 0 || max_leaf > kMaxLeafLimit) return Fail(err, "srt_bvh_build_lbvh_models: max_leaf must be in [1, 255]");
  if (n_bvhs == 0 || n_nodes == 0) return Fail(err, "scene needs at least one BVH and one node");
  if (n_tris == 0) return Fail(err, "srt_bvh_build_lbvh_models: a tree needs at least one triangle");
  if (n_tris >= kMaxTris) return Fail(err, "srt_bvh_build_lbvh_models: 2^30 triangles or more", SRT_ERR_LIMIT);
  if (bvhs[0].first_index != 0) return Fail(err, "srt_bvh_build_lbvh_models: BVH record 0's first_index is not 0");
  for (uint32_t i = 0; i < n_verts; ++i)
    for (int k = 0; k < 3; ++k)
      if (!std::isfinite(verts[i].vertex[k])) return Fail(err, "srt_bvh_build_lbvh_models: a vertex position is not finite");
  std::vector<uint32_t> owner(n_tris);
  if (int rc = OwnersFromNodes(bvhs, n_bvhs, nodes, n_nodes, n_tris, owner.data(), err)) return rc;
  const Segments seg = SegmentsOf(owner.data(), n_tris, n_bvhs);
  // box and key per record, then the stable (record, key) order
  std::vector<float> lo(3 * (size_t)n_bvhs), hi(3 * (size_t)n_bvhs);
  std::vector<uint8_t> have(n_bvhs, 0);
  for (uint32_t t = 0; t < n_tris; ++t) {
    const uint32_t r = owner[t];
    for (int k = 0; k < 3; ++k) {
      float mn, mx;
      Span(tris[t], verts, n_verts, k, &mn, &mx);
      lo[3 * (size_t)r + k] = have[r] ? refit::FoldMin(lo[3 * (size_t)r + k], mn) : mn;
      hi[3 * (size_t)r + k] = have[r] ? refit::FoldMax(hi[3 * (size_t)r + k], mx) : mx;
    }
    have[r] = 1;
  }
  std::vector<uint64_t> keys(n_tris);
  for (uint32_t t = 0; t < n_tris; ++t)
    keys[t] = RecordKey(owner[t], Key(tris[t], verts, n_verts, &lo[3 * (size_t)owner[t]], &hi[3 * (size_t)owner[t]]));
  const std::vector<uint32_t> sorted = SortByKey(keys, tris, tris_out, order_out);
  // the hierarchy per segment, a block of nodes per record
  size_t base = 0;
  for (uint32_t r = 0; r < n_bvhs; ++r) {
    if (seg.count[r] == 0) return Fail(err, kEmptyRecord);  // (unreachable after OwnersFromNodes: every root reaches a leaf)
    bvhs_out[r] = bvhs[r];
    bvhs_out[r].first_index = (uint32_t)base;
    base += PutSegment(sorted.data(), seg.first[r], seg.count[r], max_leaf, base, nodes_out);
  }
  *n_nodes_out = (uint32_t)base;
  return refit::RefitNodes(bvhs_out, n_bvhs, nodes_out, (uint32_t)base, tris_out, n_tris, verts, n_verts, err);
}

int CheckEnableModels(bool have_object, bool refit, uint32_t first_index, uint32_t n_tris, std::string* err) {
  if (!have_object) return Fail(err, "srt_query_enable_rebuild_models: null object");
  if (!refit) return Fail(err, "srt_query_enable_rebuild_models: the object was created without SRT_QUERY_REFIT");
  if (first_index != 0) return Fail(err, "srt_query_enable_rebuild_models: BVH record 0's first_index is not 0");
  if (n_tris >= kMaxTris) return Fail(err, "srt_query_enable_rebuild_models: 2^30 triangles or more", SRT_ERR_LIMIT);
  return SRT_OK;
}

bool ModelsSummaryValid(uint32_t m, uint32_t largest, uint32_t karras_pairs, uint32_t max_leaf) {
  return m <= karras_pairs && (m >= 1) == (karras_pairs >= 1) && largest <= max_leaf && (m == 0 || largest >= 1);
}

bool ScheduleFromCounts(const uint32_t* counts, int n_counts, uint32_t n_pairs, refit::Schedule* out) {
  refit::Schedule s;
  uint32_t heights = 0;
  while (heights < (uint32_t)n_counts && counts[heights] > 0) ++heights;
  uint64_t total = 0;
  for (int h = 0; h < n_counts; ++h) total += counts[h];
  refit::CloseLevels(counts, heights, true, &s);
  if (total != n_pairs || s.first[heights] != n_pairs) return false;  // a gap, or pairs that never arrived
  *out = std::move(s);
  return true;
}

}  // namespace rebuild
}  // namespace srt
