// rebuild.hpp -- the kernels of the device rebuild (include/srt_rebuild.h, srt_rebuild_leaf.h, srt_rebuild_models.h) over
// query_host.hpp's layout.  The sorts and the scan between them are hipcub's, and the boxes and triangle records are
// refit.hpp's kernels over the schedule made here.
//
// Record r owns the positions [s_r, s_r + n_r) of the sorted order, its segment, and the hierarchy is built per segment.
// One record is the segment [0, n) known at compile time: every kernel that needs a position's segment is one body with
// a template flag SEG, whose false instance loads nothing for it (segment_of).  Only the front differs in kind:
//   one record: box_partial_kernel / box_final_kernel, the scene box by a two-stage min / max reduction, and 30-bit keys;
//   several: seg_box_kernel, a box per record by atomics, and 64-bit (record, key) keys whose sort keeps the segments.
//
// keys_kernel: one lane per triangle in creation order; its Morton key in its record's box and its own index as the
//   sort's value.
// permute_kernel: one lane per position; the 16-B index triple of the triangle sorted there (SEG: and the sorted keys'
//   low dwords, which the hierarchy reads).
// karras_kernel (max_leaf 1): one lane per position.  The lane of a segment's first position writes the record's root
//   (put_root: and the ghost root beside record 0) and marks the root's parent word kNoOwner; the lane of Karras node i
//   writes the .w fields of pair i's four records (the boxes are the refit's) and the parents of its two children.  Pair
//   and node indices are global -- record r's node k is pair s_r + k -- so the last index of every segment is an unused
//   pair, kept zero.
// range_kernel, hipcub's exclusive scan, emit_kernel (max_leaf > 1) stand in for karras_kernel, and the LEAF instances of
//   climb_kernel and schedule_kernel work in rank space over the m pairs the scan counted -- m stays on the device
//   (leafsum[0]) until the rebuild's one readback.
//   range_kernel: one lane per position; its node's split (first, last, gamma) and whether it survives the collapse, and
//     the position marked as owned by no pair.
//   emit_kernel: the lane of a segment's first position writes the root, a leaf (s, c) or pair rank(s); the lane of a
//     surviving node the .w fields of pair rank(i), the parents of its internal children in rank space, the owning pair
//     of each leaf's first position, and the block's largest leaf count through one atomic max.  Only the first position
//     of a leaf starts a climb; the marks of every other position stay.
// root_leaf_kernel: one record of n <= max_leaf triangles; the leaf root (0, n).
// climb_kernel: one lane per leaf climbs towards its record's root.  At a node it exchanges its side's value into the
//   node's arrival word: the first arriver reads 0 back and stops, the second reads the other side's value -- the word
//   itself carries what is handed over, nothing else written in this launch is read in it -- computes the pair's height
//   and goes on; a root's parent word is kNoOwner, which is no pair.  No lane waits, spins or polls on another; the
//   climb is bounded by the depth.
// schedule_kernel: a counting sort of the pairs by height into the format refit.hpp reads (the order inside a
//   height is free); a block takes its share of each height with one atomic per height.
// remap_kernel: one lane per hit; the position srt_query_closest reported becomes the creation index.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "ordered_word.hpp"
#include "rebuild_rule.hpp"
#include "refit_fold.hpp"

namespace srt {
namespace rebuild {

constexpr uint32_t kBlock = 256;
constexpr uint32_t kBoxBlocks = 256;  // most partial boxes of the first stage (the second is one block)
constexpr uint32_t kMissTri = 0xFFFFFFFFu;

struct BParams {
  float4* pairs;            // 4 float4 per sibling pair (n_tris - 1 of them)
  float4* roots;            // 2 float4 per root record, n_records + 1 records (the last is the ghost root)
  const uint4* triples0;    // creation order: v0, v1, v2, material
  uint4* triples;           // sorted order
  const float4* verts;      // 2 float4 per srt_vertex
  uint32_t* vals_in;        // creation order: the sort's values
  const uint32_t* keys;     // sorted
  const uint32_t* order;    // sorted: position -> creation index
  uint32_t* parent;         // [0, n - 1): of pairs (kNoOwner: a record's root); [n - 1, 2n - 1): of leaf positions
  uint32_t* arrive;         // n - 1 arrival words, zero at launch
  uint32_t* height;         // n - 1
  uint32_t* counts;         // kHeightBins pairs per height, zero at launch
  uint32_t* cursor;         // kHeightBins, zero at launch
  uint32_t* schedule;       // n - 1 pair indices by height
  uint32_t n_verts, n_tris, n_records;
  // one record only (null / 0 otherwise)
  float* box_partial;       // 8 floats per block of the first stage: lo xyz, -, hi xyz, -
  float* box;               // 8 floats
  uint32_t* keys_in;        // creation order
  uint32_t box_blocks;
  // max_leaf > 1 only (null / 0 otherwise); then `parent` is [0, n - 1): of pairs, by rank; [n - 1, 2n - 1): the pair
  // that owns the leaf starting at the position, or kNoOwner
  uint4* split;             // n - 1: first, last, gamma, survives
  uint32_t* flags;          // n: survives, and a 0 past the last node so that the scan's last output is m
  const uint32_t* rank;     // n: the exclusive sum of flags; rank[n - 1] == m
  uint32_t* leafsum;        // m, the largest leaf count
  uint32_t max_leaf;
  // two records or more only (null otherwise); `keys` is then what permute_kernel unpacked
  const uint32_t* owner;    // n: creation index -> record
  const uint32_t* pos_rec;  // n: position -> record (the segments never move)
  const uint2* seg;         // per record: s_r, n_r
  uint32_t* seg_box;        // 8 per record: ~ordered(lo) xyz, -, ordered(hi) xyz, -; zero at launch, atomic max
  uint64_t* keys64_in;      // creation order: (record << 32) | morton
  const uint64_t* keys64;   // sorted
  uint32_t* keys_out;       // sorted: the low dwords (what `keys` points to)
};

constexpr uint32_t kNoOwner = 0xFFFFFFFFu;  // (not below any pair count: such a position starts no climb)

// A pair (or Karras node) index is < n - 1 and a position is < n by construction; the clamps keep every load and store
// inside its array whatever the device arrays hold (n >= 2).
__device__ __forceinline__ uint32_t pair_index(const BParams& bp, uint32_t x) { return x < bp.n_tris - 1u ? x : bp.n_tris - 2u; }

__device__ __forceinline__ uint32_t leaf_pos(const BParams& bp, uint32_t x) { return x < bp.n_tris ? x : bp.n_tris - 1u; }

// The word of `parent` that belongs to a child reference: of a pair, or of the leaf that starts at a position.
__device__ __forceinline__ uint32_t parent_slot(const BParams& bp, uint32_t index, bool leaf) {
  return leaf ? bp.n_tris - 1u + leaf_pos(bp, index) : pair_index(bp, index);
}

struct Span3 {
  float lo[3], hi[3];
};

// min / max over the triangle's three vertices (values only: rule 1).
__device__ __forceinline__ Span3 tri_span(const BParams& bp, uint32_t t) {
  const uint4 idx = bp.triples0[t];
  const float4 a = refit::load_pos(bp.verts, bp.n_verts, idx.x), b = refit::load_pos(bp.verts, bp.n_verts, idx.y),
               c = refit::load_pos(bp.verts, bp.n_verts, idx.z);
  refit::Box box;
  box.lo[0] = box.hi[0] = a.x;
  box.lo[1] = box.hi[1] = a.y;
  box.lo[2] = box.hi[2] = a.z;
  refit::fold(box, b);
  refit::fold(box, c);
  Span3 s;
  for (int k = 0; k < 3; ++k) {
    s.lo[k] = box.lo[k];
    s.hi[k] = box.hi[k];
  }
  return s;
}

__device__ __forceinline__ void span_merge(Span3& s, const Span3& o) {
  for (int k = 0; k < 3; ++k) {
    s.lo[k] = o.lo[k] < s.lo[k] ? o.lo[k] : s.lo[k];
    s.hi[k] = o.hi[k] > s.hi[k] ? o.hi[k] : s.hi[k];
  }
}

// The block's merged span in every lane of wave 0 (all 256 lanes call it; `have`: the lane holds a span).
__device__ __forceinline__ Span3 block_span(Span3 s, bool have, const Span3& neutral) {
  __shared__ float sh[kBlock / 64][6];
  if (!have) s = neutral;
  for (int off = 32; off > 0; off >>= 1) {
    Span3 o;
    for (int k = 0; k < 3; ++k) {
      o.lo[k] = __shfl_xor(s.lo[k], off, 64);
      o.hi[k] = __shfl_xor(s.hi[k], off, 64);
    }
    span_merge(s, o);
  }
  const uint32_t wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63u) == 0u)
    for (int k = 0; k < 3; ++k) {
      sh[wave][k] = s.lo[k];
      sh[wave][3 + k] = s.hi[k];
    }
  __syncthreads();
  for (int k = 0; k < 3; ++k) {
    s.lo[k] = sh[0][k];
    s.hi[k] = sh[0][3 + k];
  }
  for (uint32_t w = 1; w < kBlock / 64; ++w) {
    Span3 o;
    for (int k = 0; k < 3; ++k) {
      o.lo[k] = sh[w][k];
      o.hi[k] = sh[w][3 + k];
    }
    span_merge(s, o);
  }
  return s;
}

// -- the front: the box of every record, the keys --------------------------------------------------------------------------
// Stage 1: block b folds triangles b * 256 + lane, + box_blocks * 256, ...; triangle 0's span is the neutral
// element (it is part of the result anyway), so no infinity enters.
__global__ __launch_bounds__(256) void box_partial_kernel(BParams bp) {
  const Span3 neutral = tri_span(bp, 0);
  Span3 s = neutral;
  for (uint64_t t = (uint64_t)blockIdx.x * kBlock + threadIdx.x; t < bp.n_tris; t += (uint64_t)bp.box_blocks * kBlock)
    span_merge(s, tri_span(bp, (uint32_t)t));
  s = block_span(s, true, neutral);
  if (threadIdx.x == 0) {
    float* o = bp.box_partial + 8 * (size_t)blockIdx.x;
    for (int k = 0; k < 3; ++k) {
      o[k] = s.lo[k];
      o[4 + k] = s.hi[k];
    }
  }
}

// Stage 2: one block over the box_blocks <= 256 partial boxes.
__global__ __launch_bounds__(256) void box_final_kernel(BParams bp) {
  Span3 neutral;
  for (int k = 0; k < 3; ++k) {
    neutral.lo[k] = bp.box_partial[k];
    neutral.hi[k] = bp.box_partial[4 + k];
  }
  Span3 s = neutral;
  const bool have = threadIdx.x < bp.box_blocks;
  if (have) {
    const float* p = bp.box_partial + 8 * (size_t)threadIdx.x;
    for (int k = 0; k < 3; ++k) {
      s.lo[k] = p[k];
      s.hi[k] = p[4 + k];
    }
  }
  s = block_span(s, have, neutral);
  if (threadIdx.x == 0)
    for (int k = 0; k < 3; ++k) {
      bp.box[k] = s.lo[k];
      bp.box[4 + k] = s.hi[k];
    }
}

// seg_box_kernel: one lane per triangle; the box of its owner.  Floats go through the order-preserving map to uint32, the
//   lower bounds complemented, so every bound is an atomic max over words zeroed at launch: min and max of values are
//   exact and commute, no neutral element and no infinity is needed, and a record's box holds its own triangles only.  A
//   block whose triangles all have one owner folds in the block first and issues six atomics.  (ordered / unordered:
//   ordered_word.hpp.)
__device__ __forceinline__ uint32_t owner_of(const BParams& bp, uint32_t t) {
  const uint32_t r = bp.owner[t];
  return r < bp.n_records ? r : bp.n_records - 1u;
}

__global__ __launch_bounds__(256) void seg_box_kernel(BParams bp) {
  __shared__ uint32_t first_owner;
  const uint32_t t0 = blockIdx.x * kBlock;  // (< n_tris: the grid is ceil(n / 256) blocks)
  const uint32_t t = t0 + threadIdx.x;
  const bool have = t < bp.n_tris;
  const uint32_t r = owner_of(bp, have ? t : t0);
  if (threadIdx.x == 0) first_owner = r;
  __syncthreads();
  const uint32_t r0 = first_owner;
  const bool one_owner = __syncthreads_and(r == r0) != 0;  // block-uniform
  Span3 s = tri_span(bp, have ? t : t0);
  bool store = have;
  if (one_owner) {
    s = block_span(s, have, tri_span(bp, t0));
    store = threadIdx.x == 0;
  }
  if (store) {
    uint32_t* o = bp.seg_box + 8 * (size_t)r;
    for (int k = 0; k < 3; ++k) {
      atomicMax(o + k, ~ordered(s.lo[k]));
      atomicMax(o + 4 + k, ordered(s.hi[k]));
    }
  }
}

// SEG: the key in the owner's box, the owner in the high dword.
template <bool SEG>
__global__ __launch_bounds__(256) void keys_kernel(BParams bp) {
  const uint32_t t = blockIdx.x * kBlock + threadIdx.x;
  if (t >= bp.n_tris) return;
  const uint32_t r = SEG ? owner_of(bp, t) : 0u;
  const Span3 s = tri_span(bp, t);
  uint32_t q[3];
  for (int k = 0; k < 3; ++k) {
    float lo, hi;
    if (SEG) {
      const uint32_t* e = bp.seg_box + 8 * (size_t)r;
      lo = unordered(~e[k]);
      hi = unordered(e[4 + k]);
    } else {
      lo = bp.box[k];
      hi = bp.box[4 + k];
    }
    q[k] = Cell(lo, hi, s.lo[k], s.hi[k]);
  }
  const uint32_t key = Morton(q[0], q[1], q[2]);
  if (SEG) bp.keys64_in[t] = RecordKey(r, key);
  else bp.keys_in[t] = key;
  bp.vals_in[t] = t;
}

template <bool SEG>
__global__ __launch_bounds__(256) void permute_kernel(BParams bp) {
  const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
  if (p >= bp.n_tris) return;
  if (SEG) bp.keys_out[p] = (uint32_t)bp.keys64[p];
  const uint32_t src = bp.order[p];
  bp.triples[p] = bp.triples0[src < bp.n_tris ? src : 0u];  // (a whole record: one 16-B load, one 16-B store)
}

// -- the hierarchy --------------------------------------------------------------------------------------------------------
// The segment of position i (< n): s <= i < s + c <= n whatever the device arrays hold.  Without SEG it is [0, n) of
// record 0, and nothing is loaded.
struct Segment {
  uint32_t r, s, c;
};

template <bool SEG>
__device__ __forceinline__ Segment segment_of(const BParams& bp, uint32_t i) {
  Segment g{0u, 0u, bp.n_tris};
  if (SEG) {
    g.r = bp.pos_rec[i];
    g.r = g.r < bp.n_records ? g.r : bp.n_records - 1u;
    const uint2 sc = bp.seg[g.r];
    g.s = sc.x <= i ? sc.x : i;
    g.c = sc.y <= bp.n_tris - g.s ? sc.y : bp.n_tris - g.s;
    g.c = i - g.s < g.c ? g.c : i - g.s + 1u;
  }
  return g;
}

// One reference, the .w fields of a record of two float4 (the bounds are the refit's to write): a pair index and 0, or
// a leaf's first position and its count.
__device__ __forceinline__ void put_ref(float4* rec, uint32_t ref, uint32_t count) {
  rec[0] = make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(ref));
  rec[1] = make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(count));
}

// Root record r, and the ghost root (record n_records) beside record 0.
__device__ __forceinline__ void put_root(const BParams& bp, uint32_t r, uint32_t ref, uint32_t count) {
  put_ref(bp.roots + 2 * (size_t)r, ref, count);
  if (r == 0u) put_ref(bp.roots + 2 * (size_t)bp.n_records, ref, count);
}

template <bool SEG>
__global__ __launch_bounds__(256) void karras_kernel(BParams bp) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  const uint32_t n = bp.n_tris;  // >= 2
  if (i >= n) return;
  const Segment g = segment_of<SEG>(bp, i);
  if (i == g.s) {  // a root pair climbs no further; a leaf root's position starts no climb
    const Slot root = SegmentRoot(g.s, g.c, 1u);
    put_root(bp, g.r, root.index, root.count);
    bp.parent[parent_slot(bp, i, root.count > 0u)] = kNoOwner;
  }
  if (i + 1u >= n) return;  // (no pair slot n - 1)
  float4* rec = bp.pairs + 4 * (size_t)i;
  if (i - g.s + 1u >= g.c) {  // the last index of a segment: unused, kept zero
    for (int k = 0; k < 4; ++k) rec[k] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    return;
  }
  const Split sp = SegmentSplit(bp.keys, g.s, g.c, i);
  const Child l{(uint32_t)sp.gamma, sp.first == sp.gamma}, r{(uint32_t)(sp.gamma + 1), sp.last == sp.gamma + 1};
  put_ref(rec, l.index, l.leaf ? 1u : 0u);
  put_ref(rec + 2, r.index, r.leaf ? 1u : 0u);
  bp.parent[parent_slot(bp, l.index, l.leaf)] = i;
  bp.parent[parent_slot(bp, r.index, r.leaf)] = i;
}

// -- max_leaf > 1 ------------------------------------------------------------------------------------------------------
template <bool SEG>
__global__ __launch_bounds__(256) void range_kernel(BParams bp) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  const uint32_t n = bp.n_tris;  // >= 2
  if (i >= n) return;
  if (i == 0) bp.leafsum[1] = 0u;  // the emit kernel's atomic max starts here
  bp.parent[n - 1 + i] = kNoOwner;
  const Segment g = segment_of<SEG>(bp, i);
  uint4 out = make_uint4(0u, 0u, 0u, 0u);  // a leaf root's segment has no node, nor has a segment's last index
  if (g.c > bp.max_leaf && i - g.s + 1u < g.c) {
    const Split sp = SegmentSplit(bp.keys, g.s, g.c, i);
    out = make_uint4((uint32_t)sp.first, (uint32_t)sp.last, (uint32_t)sp.gamma, Survives(sp, bp.max_leaf) ? 1u : 0u);
  }
  if (i + 1u < n) bp.split[i] = out;
  bp.flags[i] = out.w;
}

// One slot of pair r.
__device__ __forceinline__ uint32_t emit_slot(const BParams& bp, float4* rec, const Slot& s, uint32_t r) {
  const bool leaf = s.count > 0u;
  const uint32_t ref = leaf ? leaf_pos(bp, s.index) : pair_index(bp, bp.rank[pair_index(bp, s.index)]);
  put_ref(rec, ref, s.count);
  bp.parent[parent_slot(bp, ref, leaf)] = r;
  return s.count;
}

template <bool SEG>
__global__ __launch_bounds__(256) void emit_kernel(BParams bp) {
  __shared__ uint32_t largest;
  if (threadIdx.x == 0) largest = 0u;
  __syncthreads();
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  const uint32_t n = bp.n_tris;
  if (i == 0) bp.leafsum[0] = bp.rank[n - 1u];  // m for the kernels after
  if (i < n) {
    const Segment g = segment_of<SEG>(bp, i);
    if (i == g.s) {
      const Slot root = SegmentRoot(g.s, g.c, bp.max_leaf);
      if (root.count > 0u) {
        put_root(bp, g.r, root.index, root.count);
      } else {  // node s survives: c > max_leaf
        const uint32_t rr = pair_index(bp, bp.rank[pair_index(bp, i)]);
        put_root(bp, g.r, rr, 0u);
        bp.parent[rr] = kNoOwner;
      }
    }
  }
  if (i + 1 < n) {
    const uint4 sp4 = bp.split[i];
    if (sp4.w != 0u) {
      Split sp;
      sp.first = sp4.x;
      sp.last = sp4.y;
      sp.gamma = sp4.z;
      const uint32_t r = pair_index(bp, bp.rank[i]);
      float4* rec = bp.pairs + 4 * (size_t)r;
      const uint32_t a = emit_slot(bp, rec, LeftSlot(sp, bp.max_leaf), r);
      const uint32_t b = emit_slot(bp, rec + 2, RightSlot(sp, bp.max_leaf), r);
      if ((a > b ? a : b) > 0u) atomicMax(&largest, a > b ? a : b);
    }
  }
  __syncthreads();  // (every lane arrives)
  if (threadIdx.x == 0 && largest != 0u) atomicMax(bp.leafsum + 1, largest);
}

__global__ __launch_bounds__(256) void root_leaf_kernel(BParams bp) {
  if (blockIdx.x == 0 && threadIdx.x == 0) put_root(bp, 0u, 0u, bp.n_tris);
}

// -- the heights and the schedule ------------------------------------------------------------------------------------------
// The pairs of the tree being built: n - 1, or with LEAF the m the scan counted (never more than n - 1).
template <bool LEAF>
__device__ __forceinline__ uint32_t pair_count(const BParams& bp) {
  if (!LEAF) return bp.n_tris - 1u;
  const uint32_t m = bp.leafsum[0];
  return m < bp.n_tris - 1u ? m : bp.n_tris - 1u;
}

template <bool LEAF>
__global__ __launch_bounds__(256) void climb_kernel(BParams bp) {
  __shared__ uint32_t bins[kHeightBins];
  if (threadIdx.x < kHeightBins) bins[threadIdx.x] = 0u;
  __syncthreads();
  const uint32_t n = bp.n_tris;  // >= 2
  const uint32_t n_pairs = pair_count<LEAF>(bp);
  const uint32_t leaf = blockIdx.x * kBlock + threadIdx.x;  // (LEAF: a position; the first of a leaf has an owner)
  if (leaf < n) {
    uint32_t p = bp.parent[n - 1 + leaf];
    uint32_t val = 0u;  // of a child: 0 for a leaf, its pair's height + 1 for an internal node
    for (int step = 0; step < kHeightBins && p < n_pairs; ++step) {  // (a root's parent is kNoOwner)
      const uint32_t old = __hip_atomic_exchange(bp.arrive + p, val + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (old == 0u) break;  // the first to arrive: the other side's lane carries on from here
      uint32_t h = old - 1u > val ? old - 1u : val;
      h = h < (uint32_t)kHeightBins ? h : (uint32_t)kHeightBins - 1u;  // (the depth bound keeps it below)
      bp.height[p] = h;
      atomicAdd(&bins[h], 1u);
      val = h + 1u;
      p = bp.parent[p];
    }
  }
  __syncthreads();  // (every lane arrives: the climb above waits for nothing)
  if (threadIdx.x < kHeightBins && bins[threadIdx.x] != 0u) atomicAdd(bp.counts + threadIdx.x, bins[threadIdx.x]);
}

// SEG without LEAF: the pair array has unused slots (the last index of every segment); a pair exists iff both its
// children arrived, which left its arrival word non-zero.
template <bool LEAF, bool SEG>
__global__ __launch_bounds__(256) void schedule_kernel(BParams bp) {
  __shared__ uint32_t bins[kHeightBins], base[kHeightBins];
  if (threadIdx.x < kHeightBins) bins[threadIdx.x] = 0u;
  __syncthreads();
  const uint32_t n_pairs = pair_count<LEAF>(bp);
  const uint32_t p = blockIdx.x * kBlock + threadIdx.x;
  uint32_t h = 0u, rank = 0u;
  const bool exists = p < n_pairs && (LEAF || !SEG || bp.arrive[p] != 0u);
  if (exists) {
    h = bp.height[p];
    h = h < (uint32_t)kHeightBins ? h : (uint32_t)kHeightBins - 1u;
    rank = atomicAdd(&bins[h], 1u);
  }
  __syncthreads();
  if (threadIdx.x < kHeightBins && bins[threadIdx.x] != 0u) {
    uint32_t first = 0u;  // of this height: the pairs of the heights under it
    for (uint32_t k = 0; k < threadIdx.x; ++k) first += bp.counts[k];
    base[threadIdx.x] = first + atomicAdd(bp.cursor + threadIdx.x, bins[threadIdx.x]);
  }
  __syncthreads();
  if (exists) {
    const uint32_t at = base[h] + rank;
    if (at < n_pairs) bp.schedule[at] = p;
  }
}

// hits: 2 uint4 per srt_hit; the first dword is the triangle.
__global__ __launch_bounds__(256) void remap_kernel(uint32_t* hits, const uint32_t* order, uint32_t n, uint32_t n_tris) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  uint32_t* tri = hits + 8 * (size_t)i;
  const uint32_t pos = *tri;
  if (pos != kMissTri && pos < n_tris) *tri = order[pos];
}

}  // namespace rebuild
}  // namespace srt
