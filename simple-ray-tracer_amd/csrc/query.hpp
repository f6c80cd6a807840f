// query.hpp -- query_kernel: batched closest-hit / any-hit ray queries (include/srt_query.h).
//
// The shape is sample_kernel's without the shading: persistent 256-lane blocks, each
// wave claiming runs of rays from a launch-wide counter; per-lane resumable traversal (current node in
// registers, stack in LDS, or in HBM for deep trees); and an intra-wave refill: when fewer than
// `refill_min` lanes of a wave still traverse, the finished lanes write their results and take the next
// rays of the wave's run, ranked by a ballot and a prefix count.  The arithmetic is traversal.hpp's
// (box_t / box_test / tri_prep / tri_finish / xform / recip_exact: contract A), read-only; the scene is
// query_host.hpp's layout.  No counters.
#pragma once

#include "traversal.hpp"

namespace srt {
namespace query {
using namespace dev;

struct QParams {
  const float4* pairs;   // 4 float4 per sibling pair
  const float4* roots;   // 2 float4 per BVH record, n_bvhs + 1 records (the last: node 0)
  const float4* tris;    // 3 float4 per triangle
  const float* frames;   // 16 floats per BVH record, n_bvhs + 1 records (the last: zeros)
  const float4* rays;    // 2 float4 per ray
  void* out;             // srt_hit[n] (closest) or uint8_t[n] (any)
  uint32_t* ctr;         // next unclaimed ray of the launch (zeroed before it)
  uint32_t* gstack;      // HBM stacks: one area of 256 * F * stack_entries dwords per block
  uint32_t n;
  uint32_t n_bvhs, bvh_count;
  uint32_t claim;        // rays a wave claims per atomic (a multiple of 64)
  int stack_entries;
  int refill_min;        // a wave refills when fewer lanes than this traverse (1..64)
  const uint32_t* order; // ORDER instances only: position in the launch -> ray index, a permutation of 0 .. n-1
};

#ifndef SRT_QUERY_SUBSTEPS
#define SRT_QUERY_SUBSTEPS 6
#endif
constexpr int kSubSteps = SRT_QUERY_SUBSTEPS;  // traversal sub-steps between two refill checks
constexpr uint32_t kMiss = 0xFFFFFFFFu;

// Per-lane traversal state.  cnt tells the states apart as Trav's does: (int)cnt > 0 leaf (ref: next
// triangle), cnt == 0 internal (ref: its child pair), cnt == kNoneCnt nothing current (pop next).  A lane
// without a ray has cnt == kNoneCnt and sp == 0, so no sub-step touches it.
struct QLane {
  f3 o, d, inv;
  float dist;
  uint32_t ref, cnt, hit, hit_bvh, bi, idx;
  int sp;
};

template <bool PACK>
struct Stack {
  uint32_t* base;  // this lane's column; field k of entry s at base[(F * s + k) * 256]
  static constexpr int F = PACK ? 2 : 3;
  __device__ __forceinline__ void write(int s, uint32_t ref, uint32_t cnt, float t) const {
    slot_write<PACK>(base, kBlock256, s, ref, cnt, t);
  }
  __device__ __forceinline__ void read(int s, uint32_t& ref, uint32_t& cnt, float& t) const {
    slot_read<PACK>(base, kBlock256, s, ref, cnt, t);
  }
  static constexpr int kBlock256 = 256;
};

// The ray enters BVH record L.bi: the reference's per-model transform and the root's box test.
__device__ __forceinline__ void begin_bvh(const QParams& qp, QLane& L) {
  const uint32_t b = L.bi < qp.n_bvhs ? L.bi : qp.n_bvhs;  // past n_bvhs: zero frame, node 0
  const float4 r0 = qp.rays[2 * (size_t)L.idx], r1 = qp.rays[2 * (size_t)L.idx + 1];
  const float* m = qp.frames + 16 * (size_t)b;
  L.o = xform(m, mk(r0.x, r0.y, r0.z), 1.0f);
  L.d = xform(m, mk(r1.x, r1.y, r1.z), 0.0f);
  L.inv = mk(recip_exact(L.d.x), recip_exact(L.d.y), recip_exact(L.d.z));
  const float4 rlo = qp.roots[2 * (size_t)b], rhi = qp.roots[2 * (size_t)b + 1];
  const bool ok = box_ok(box_t(L.o, L.inv, rlo, rhi), L.dist);
  L.ref = __float_as_uint(rlo.w);
  L.cnt = ok ? __float_as_uint(rhi.w) : kNoneCnt;
  L.sp = 0;
}

// Internal node: both children's boxes; the left child is stacked when both pass (its slot is written
// either way: the stack holds depth + 1 entries), the right child is visited first.
template <bool PACK>
__device__ __forceinline__ void step_internal(const QParams& qp, const Stack<PACK>& stk, QLane& L) {
  const float4* p = qp.pairs + 4 * (size_t)L.ref;
  const float4 l0 = p[0], h0 = p[1], l1 = p[2], h1 = p[3];
  float b0, b1;
  const bool v0 = box_test(L.o, L.inv, l0, h0, L.dist, b0);
  const bool v1 = box_test(L.o, L.inv, l1, h1, L.dist, b1);
  const uint32_t r0 = __float_as_uint(l0.w), n0 = __float_as_uint(h0.w);
  stk.write(L.sp, r0, n0, b0);
  L.sp += (v0 & v1) ? 1 : 0;
  L.ref = v1 ? __float_as_uint(l1.w) : r0;
  L.cnt = v1 ? __float_as_uint(h1.w) : (v0 ? n0 : kNoneCnt);
}

// Leaf: its next two triangles in order, each against the distance the previous one left (a one-triangle
// leaf reads the record after it, or the pad record, and discards it).  Returns true when an any-hit ray
// accepted a triangle and stops.
template <bool ANY>
__device__ __forceinline__ bool step_leaf(const QParams& qp, QLane& L) {
  const float4* tp = qp.tris + 3 * (size_t)L.ref;
  const float4 a0 = tp[0], a1 = tp[1], a2 = tp[2], c0 = tp[3], c1 = tp[4], c2 = tp[5];
  TriPrep p0, p1;
  bool slow = tri_prep(L.d, a0, a1, a2, p0);
  slow |= tri_prep(L.d, c0, c1, c2, p1);
  if (__builtin_expect(slow, 0)) {
    p0.f = 1.0f / p0.a;
    p1.f = 1.0f / p1.a;
  }
  float t0, t1;
  const bool k0 = tri_finish(L.o, L.d, p0, L.dist, t0);
  L.dist = k0 ? t0 : L.dist;
  L.hit = k0 ? L.ref : L.hit;
  const bool two = L.cnt > 1u;
  const bool k1 = two & !(ANY & k0) & tri_finish(L.o, L.d, p1, L.dist, t1);
  L.dist = k1 ? t1 : L.dist;
  L.hit = k1 ? L.ref + 1u : L.hit;
  L.hit_bvh = (k0 | k1) ? L.bi : L.hit_bvh;
  const uint32_t n = two ? 2u : 1u;
  const bool stop = ANY & (k0 | k1);
  const uint32_t rest = L.cnt - n;
  L.ref += n;
  L.cnt = (rest == 0u || stop) ? kNoneCnt : rest;
  L.sp = stop ? 0 : L.sp;
  return stop;
}

// Nothing current: pop one entry; it is visited if it still beats the running distance.
template <bool PACK>
__device__ __forceinline__ void step_pop(const Stack<PACK>& stk, QLane& L) {
  if ((L.cnt == kNoneCnt) & (L.sp > 0)) {
    --L.sp;
    uint32_t r, n;
    float et;
    stk.read(L.sp, r, n, et);
    L.ref = r;
    L.cnt = et < L.dist ? n : kNoneCnt;
  }
}

// The finished ray's record, as two dwordx4 stores (closest), or one byte (any).
template <bool ANY>
__device__ __forceinline__ void write_result(const QParams& qp, const QLane& L) {
  if constexpr (ANY) {
    static_cast<uint8_t*>(qp.out)[L.idx] = L.hit != kMiss ? 1 : 0;
  } else {
    uint4 a = make_uint4(kMiss, __float_as_uint(L.dist), 0u, 0u), b = make_uint4(0u, 0u, 0u, 0u);
    if (L.hit != kMiss) {
      const float4* tp = qp.tris + 3 * (size_t)L.hit;
      const float4 A = tp[0], B = tp[1], C = tp[2];
      const f3 nrm = normalize(cross(mk(A.w, B.x, B.y), mk(B.z, B.w, C.x)));
      a = make_uint4(L.hit, __float_as_uint(L.dist), __float_as_uint(nrm.x), __float_as_uint(nrm.y));
      b = make_uint4(__float_as_uint(nrm.z), __float_as_uint(C.y), L.hit_bvh, 0u);
    }
    uint4* o = static_cast<uint4*>(qp.out) + 2 * (size_t)L.idx;
    o[0] = a;
    o[1] = b;
  }
}

// ORDER (include/srt_query_sort.h): the claimed positions [cur, end) are positions of qp.order, and a refilled lane
// takes the ray sorted there; rays are read and results written in place through L.idx, as without it.
template <bool ANY, bool HBM, bool PACK, bool ORDER = false>
__global__ __launch_bounds__(256) void query_kernel(QParams qp) {
  const uint32_t lane = threadIdx.x & 63u;
  Stack<PACK> stk;
  if constexpr (HBM)
    stk.base = qp.gstack + (size_t)blockIdx.x * (256u * (uint32_t)Stack<PACK>::F * (uint32_t)qp.stack_entries) +
               threadIdx.x;
  else stk.base = reinterpret_cast<uint32_t*>(g_smem) + threadIdx.x;
  QLane L;
  L.o = L.d = L.inv = mk(0.0f, 0.0f, 0.0f);
  L.dist = 0.0f;
  L.ref = 0u;
  L.cnt = kNoneCnt;
  L.hit = kMiss;
  L.hit_bvh = L.bi = L.idx = 0u;
  L.sp = 0;
  bool active = false;   // the lane's ray is still traversing
  bool pending = false;  // the lane's ray is finished and its result not yet written
  uint32_t cur = 0, end = 0;  // the wave's run of claimed rays [cur, end) (wave-uniform)
  bool exhausted = false;     // the launch has no unclaimed rays left (wave-uniform)
  for (;;) {
    const int nact = __popcll(__ballot(active));
    if (nact < qp.refill_min) {
      if (pending) {
        write_result<ANY>(qp, L);
        pending = false;
      }
      bool need = !active;
      while (!exhausted) {
        const uint64_t nm = __ballot(need);
        if (nm == 0) break;
        if (cur == end) {
          uint32_t c = 0;
          if (lane == 0) c = atomicAdd(qp.ctr, qp.claim);
          c = (uint32_t)__builtin_amdgcn_readfirstlane((int)c);
          if (c >= qp.n) {
            exhausted = true;
            break;
          }
          cur = c;
          end = qp.n - c < qp.claim ? qp.n : c + qp.claim;
        }
        const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(nm >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)nm, 0u));
        const uint32_t left = end - cur, want = (uint32_t)__popcll(nm);
        if (need && rank < left) {
          if constexpr (ORDER) {
            const uint32_t r = qp.order[cur + rank];
            L.idx = r < qp.n ? r : qp.n - 1u;  // (a permutation by construction; the clamp keeps any word inside)
          } else {
            L.idx = cur + rank;
          }
          L.dist = qp.rays[2 * (size_t)L.idx + 1].w;
          L.hit = kMiss;
          L.hit_bvh = 0u;
          L.bi = 0u;
          need = false;
          if (qp.bvh_count == 0u) {
            pending = true;  // no BVH to walk: a miss with the input distance
          } else {
            active = true;
            begin_bvh(qp, L);
          }
        }
        cur += want < left ? want : left;
      }
      if (__ballot(active | pending) == 0) break;  // (only when the launch is exhausted)
    }
#pragma unroll
    for (int k = 0; k < kSubSteps; ++k) {
      if (L.cnt == 0u) {
        step_internal<PACK>(qp, stk, L);
      } else if (trav_at_leaf(L.cnt)) {
        if (step_leaf<ANY>(qp, L)) {
          active = false;
          pending = true;
        }
      }
      step_pop<PACK>(stk, L);
    }
    // nothing current and an empty stack: this BVH is done; the next one, or the ray is finished
    if (active & (L.cnt == kNoneCnt) & (L.sp == 0)) {
      if (L.bi + 1u >= qp.bvh_count) {
        active = false;
        pending = true;
      } else {
        ++L.bi;
        begin_bvh(qp, L);
      }
    }
  }
}

}  // namespace query
}  // namespace srt
