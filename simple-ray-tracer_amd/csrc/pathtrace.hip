// pathtrace.hip -- the kernel-launching part of the device context behind the C ABI (context.hpp): scene
// and texture uploads, launches of the kernels in kernels.hpp.  Only the code that talks to the device:
// context.cpp holds the host-only part of the context, launch_plan.cpp a launch's LDS layout and chunks,
// scene_image.cpp the arrays an upload sends, scene_layout.cpp the validation and the node / triangle layouts.
//
// Kernels (kernels.hpp; DESIGN.md sections 4-5):
//   sample_kernel      persistent: waves claim 64-item batches (an 8x8 tile of
//                      one frame) from a launch-wide counter; each lane runs one
//                      path sample at a time (camera ray, bounces, shadow rays)
//                      with resumable, order-exact BVH traversal, and writes the
//                      sample's radiance to an HBM sample buffer;
//   accumulate_kernel  the ordered per-pixel sum (bit-identical to per-frame
//                      image read-modify-writes) and the sRGB8 image.
// Scene residency: LDS mode copies nodes + triangles into each block's LDS
// (1024-lane blocks, packed LDS stacks); global-scene mode reads them from HBM
// through L2/MALL with an LDS ring of stack entries backed by HBM stacks.
// Device layout (re-laid from the std430 SSBOs):
//   nodes  : 32 B per node (min.xyz|first, max.xyz|count), base offset 32 B so
//            each sibling pair is one 64-B aligned block;
//   tris   : 48 B per triangle = v0, e1 = v1 - v0, e2 = v2 - v0, material id,
//            padded with kTriPad zero records;
//   mats   : 32 B shading material (albedo|roughness, specular) precomputed
//            from MaterialFromOBJ (raytrace_utils.glsl:140-175);
//   lights, noise: context.cpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstddef>
#include <cstring>
#include <string>
#include <vector>

#include "kernels.hpp"
#include "pool.hpp"
#include "wavefront.hpp"

#include "context.hpp"
#include "launch_plan.hpp"
#include "scene_image.hpp"
#include "scene_layout.hpp"
#include "tile_cull.hpp"

// ===========================================================================
// host side: the launches behind the C ABI
// ===========================================================================
using srt::EnsureBvhs, srt::EnsureLights, srt::FreeDev, srt::HipFail, srt::LocalRows, srt::Quiesce, srt::WaitLaunchIdle;
using srt::ValidateNodes;

namespace {

// The span record of the launch being set up (kernels.hpp sample_body), initialised on its stream.
int TakeSpan(srt_context* c, srt::KParams& kp) {
  if (!c->d_span) HIP_OK(hipMalloc(&c->d_span, sizeof(unsigned long long) * 2 * srt_context::kSpanCap));
  const unsigned long long seq = c->span_seq++;
  kp.span = c->d_span + 2 * (seq % srt_context::kSpanCap);
  const size_t chunk = (size_t)(c->ev_used / 2);
  if (c->chunk_span.size() <= chunk) c->chunk_span.resize(chunk + 1, -1);
  c->chunk_span[chunk] = (long long)seq;
  hipLaunchKernelGGL(srt::span_init_kernel, dim3(1), dim3(64), 0, c->lstream, kp.span);
  HIP_OK(hipGetLastError());
  return SRT_OK;
}

// The launch buffers of the context and of pipeline slot `s` trade places (in, launch, out again).
// Launches in series share the context's tile costs and order (each orders its tiles by the costs of
// the launch just before it, which has ended) and its global stacks; overlapping launches each keep
// their slot's.
void SwapSlot(srt_context* c, srt_context::Slot& s, bool own) {
  std::swap(c->d_lbuf, s.lbuf);
  std::swap(c->lbuf_bytes, s.lbuf_bytes);
  std::swap(c->d_batch_ctr, s.batch_ctr);
  std::swap(c->batch_ctr_cap, s.batch_ctr_cap);
  if (own) {
    std::swap(c->d_tile_cost, s.tile_cost);
    std::swap(c->d_tile_order, s.tile_order);
    std::swap(c->tile_cap, s.tile_cap);
    std::swap(c->tile_costs_for, s.tile_costs_for);
    std::swap(c->d_gstack, s.gstack);
    std::swap(c->gstack_bytes, s.gstack_bytes);
  }
}

// GetCamera (raytrace_compute.glsl:47-76) with focusDist = 1 (:384)
void CameraParams(const srt_context* c, srt::KParams* kp) {
  const float aspect = (float)c->W / (float)c->H;
  const float hf = (float)c->W / aspect;
  int height = (hf != hf) ? 0 : (int)hf;
  height = (height < 1) ? 1 : height;
  const float focus = 1.0f;
  const float w[3] = {-c->cam_dir[0], -c->cam_dir[1], -c->cam_dir[2]};
  float du[3], dv[3], p00[3];
  for (int i = 0; i < 3; ++i) {
    const float viewU = c->cam_right[i] * focus;
    const float viewV = c->cam_up[i] * focus;
    du[i] = viewU / (float)c->W;
    dv[i] = viewV / (float)height;
    const float ll = ((c->cam_origin[i] - focus * w[i]) - viewU / 2.0f) - viewV / 2.0f;
    p00[i] = ll + 0.5f * (du[i] + dv[i]);
  }
  kp->cx = c->cam_origin[0]; kp->cy = c->cam_origin[1]; kp->cz = c->cam_origin[2];
  kp->p00x = p00[0]; kp->p00y = p00[1]; kp->p00z = p00[2];
  kp->dux = du[0]; kp->duy = du[1]; kp->duz = du[2];
  kp->dvx = dv[0]; kp->dvy = dv[1]; kp->dvz = dv[2];
}

int FillParams(srt_context* c, srt::KParams* kp, bool need_images) {
  if (c->W <= 0 || c->H <= 0) { srt::SetError("Width/Height not set"); return SRT_ERR_STATE; }
  // sample_kernel packs a pixel as x | local_row << 16 (kernels.hpp refill)
  if (c->W > 65535 || LocalRows(c, c->H) > 32767) {
    srt::SetError("Width > 65535 or more than 32767 rows per rank");
    return SRT_ERR_LIMIT;
  }
  if (c->show_model && !c->scene_ok) { srt::SetError("showModel set but no scene uploaded"); return SRT_ERR_STATE; }
  if (need_images) {
    if (c->noise_texels != (size_t)c->W * (size_t)c->H) {
      srt::SetError("noise buffers must hold Width*Height texels");
      return SRT_ERR_STATE;
    }
    if (!c->d_accum || c->img_w != c->W || c->img_rows != LocalRows(c, c->H)) {
      srt::SetError("images not allocated for the current Width/Height/tiling (srt_alloc_images)");
      return SRT_ERR_STATE;
    }
  }
  int rc = EnsureLights(c);
  if (rc) return rc;
  if (c->show_model) {
    rc = EnsureBvhs(c);
    if (rc) return rc;
  }
  std::memset(kp, 0, sizeof(*kp));
  kp->nodes = c->d_nodes;
  kp->tris = c->d_tris;
  kp->mats = c->d_mats;
  kp->tri_uv = c->d_tri_uv;
  kp->top_f4 = 0;  // (set per launch: the fused instance's LDS copy of the top levels)
  kp->top_lds_f4 = 0;
  kp->tex_texels = static_cast<const float4*>(c->d_tex);
  kp->tex_texels8 = static_cast<const uint32_t*>(c->d_tex);
  kp->tex_info = c->d_tex_info;
  kp->n_tex = c->d_tex ? c->n_tex : 0u;
  kp->lights = c->d_lights;
  kp->bvhs = c->d_bvhs;
  kp->noise_xy = c->d_noise_xy;
  kp->noise_u = c->d_noise_u;
  kp->accum = c->d_accum;
  kp->out = c->d_out;
  kp->stats = c->d_stats;
  kp->nan_ctr = c->d_nan;
  kp->W = c->W;
  kp->H = c->H;
  kp->WH = c->W * c->H;
  kp->light_count = std::max(c->light_count, 0);
  kp->light_records = (int)c->h_lights.size();
  kp->bvh_count = c->bvh_count;
  kp->show_model = c->show_model;
  kp->max_depth = c->max_depth;
  kp->rank = c->rank;
  kp->nranks = c->nranks;
  kp->band_rows = c->band_rows;
  kp->band_shift = -1;
  for (int s = 0; s < 31; ++s)
    if ((1 << s) == c->band_rows) kp->band_shift = s;
  kp->local_rows = LocalRows(c, c->H);
  if (c->nranks > 1) {  // the row bands' global rows, one table read per new sample in the kernels
    const long long key = ((((long long)c->rank * 4096 + c->nranks) * 65536 + c->band_rows) << 20) + kp->local_rows;
    if (key != c->row_map_key) {
      std::vector<int> rows((size_t)std::max(kp->local_rows, 1));
      for (int ly = 0; ly < kp->local_rows; ++ly) {
        const int band = ly / c->band_rows;
        rows[ly] = (band * c->nranks + c->rank) * c->band_rows + (ly - band * c->band_rows);
      }
      if (int rq = Quiesce(c)) return rq;
      FreeDev(c->d_row_map);
      c->d_row_map = nullptr;
      c->row_map_key = -1;
      HIP_OK(hipMalloc(&c->d_row_map, rows.size() * sizeof(int)));
      HIP_OK(hipMemcpyAsync(c->d_row_map, rows.data(), rows.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
      HIP_OK(hipStreamSynchronize(c->stream));
      c->row_map_key = key;
      c->h_row_map = std::move(rows);
    }
    kp->row_map = c->d_row_map;
  }
  kp->local_pixels = kp->local_rows * c->W;
  kp->ext_w = c->W;
  kp->ext_h = c->H;
  kp->stack_entries = c->stack_entries;
  kp->nodes_f4 = (int)(2 * ((size_t)c->n_nodes + 1));
  kp->nodes_lds_f4 = (int)((((size_t)kp->nodes_f4 + 3) >> 2) * srt::kNodeBlkF4);  // padded pair blocks
  kp->ref_or = c->ref_or;
  kp->tris_f4 = (int)(3 * ((size_t)c->n_tris + srt::kTriPad));  // with the padding records
  CameraParams(c, kp);
  return SRT_OK;
}

// LDS mode's block (one per CU, the scene copied into its LDS): 1024 threads = 4 waves per SIMD.  An
// experiment build with 768 (3 waves per SIMD) measures what a wave per SIMD is worth
#ifndef SRT_LDS_BLOCK
#define SRT_LDS_BLOCK 1024
#endif
constexpr int kLdsBlock = SRT_LDS_BLOCK;
// Global-scene mode's block: 256 lanes, except the timed fused instance at 5 waves per SIMD, whose blocks
// hold SRT_GW5_BLOCK lanes (a multiple of 64 dividing 1280, the 20 waves 5 per SIMD make): with 640, two
// blocks per CU, so the tree's top levels are copied into LDS twice per CU instead of five times and the
// LDS a block may take beside its rings (80 KB) holds one level more
#ifndef SRT_GW5_BLOCK
#define SRT_GW5_BLOCK 256
#endif
constexpr int kGw5Block = SRT_GW5_BLOCK;
static_assert(kGw5Block % 64 == 0 && 1280 % kGw5Block == 0, "SRT_GW5_BLOCK: 64-lane waves, 1280 lanes per CU");
// This build's constants for the host-only plans (launch_plan.hpp, scene_image.hpp), which never see the
// macros behind them
constexpr srt::BuildConsts kBuild = {kLdsBlock, kGw5Block, srt::kNodeBlkF4, srt::global_ring(4), srt::global_ring(5),
                                     SRT_COOP != 0, srt::kCoopWaveBytes, srt::kCoopIdxBits, srt::kPoolTravLanes,
                                     srt::kNodePad, (uint32_t)srt::kTriPad, srt::kTreeletCnt};

// Resident blocks per CU of kernel `fn` at `block` lanes and `lds` bytes: the occupancy API's answer capped
// by the LDS allocation rule (ResidentPerCu), queried once per (kernel instance, LDS size) -- the query
// runs on the host between the launch's timing events otherwise
template <typename F>
int ResidentBlocks(srt_context* c, F* fn, int block, size_t lds, int* per_cu) {
  const void* key = reinterpret_cast<const void*>(fn);
  *per_cu = 0;
  for (const auto& e : c->occupancy)
    if (e.fn == key && e.lds == lds) *per_cu = e.per_cu;
  if (*per_cu == 0) {
    HIP_OK(hipOccupancyMaxActiveBlocksPerMultiprocessor(per_cu, fn, block, lds));
    *per_cu = srt::ResidentPerCu(*per_cu, lds);
    c->occupancy.push_back({key, lds, *per_cu});
  }
  return SRT_OK;
}

template <bool COUNT, bool LDSM, bool PACK, int BLOCK, bool TEX, bool FUSE = false, int GW = 4>
int LaunchSamples(srt_context* c, srt::KParams kp, size_t lds) {
  int per_cu = 0;
  if (int ro = ResidentBlocks(c, &srt::sample_kernel<COUNT, LDSM, PACK, BLOCK, TEX, FUSE, GW>, BLOCK, lds, &per_cu))
    return ro;
  const int blocks = c->num_cus * per_cu;
  c->launch_per_cu = per_cu;
  c->launch_block = BLOCK;
  if constexpr (!LDSM) {  // global-scene mode: every lane's full stack in HBM (backing the LDS ring)
    const size_t lanes = (size_t)blocks * BLOCK;
    const size_t need = lanes * (PACK ? 2 : 3) * sizeof(uint32_t) * (size_t)kp.stack_entries;
    if (need > c->gstack_bytes) {
      if (int rw = WaitLaunchIdle(c)) return rw;
      FreeDev(c->d_gstack);
      c->d_gstack = nullptr;
      c->gstack_bytes = 0;
      HIP_OK(hipMalloc(&c->d_gstack, need));
      c->gstack_bytes = need;
    }
    kp.gstack = c->d_gstack;
    kp.gstack_stride = (int)lanes;
  }
#ifdef SRT_WAVE_TRACE
  {  // diagnostic build: 4 realtime stamps per wave of the last launch
    const size_t need = (size_t)blocks * (BLOCK / 64) * 4 * sizeof(unsigned long long);
    if (need > c->trace_bytes) {
      FreeDev(c->d_trace);
      HIP_OK(hipMalloc(&c->d_trace, need));
      c->trace_bytes = need;
    }
    c->trace_waves = blocks * (BLOCK / 64);
    kp.wave_trace = c->d_trace;
  }
#endif
  {  // single-batch claims for the last tail_claims * kClaim batches per wave (sample_kernel; measured
     // in round 1: 2 -> 16 halves the launch's tail)
    const long long waves = (long long)blocks * (BLOCK / 64);
    const long long n_batches = (long long)kp.live_tiles * kp.nframes;
    const int tail_claims = (FUSE && GW == 5 && !TEX) ? c->tail_claims_gw5 : c->tail_claims;
    kp.tail_start = (int)std::max<long long>(0, n_batches - (long long)tail_claims * srt::kClaim * waves);
  }
  // the early-break threshold of the fused 4-wave instance (trees of 48-600 MB): 7, where the
  // latency-bound soups gain (1 M: 1,370 -> 1,413-1,418 Mrays/s; 3 M: 939 -> 971) and the 5-wave
  // (torus knot) and IL (C5) instances lose
  if constexpr (!LDSM && FUSE && GW == 4)
    if (!c->trav_frac16_global_env) kp.trav_frac16 = 7;
  // ... and of the timed IL instance (trees past 600 MB): 8 (C5, kernel ms on one box: 9 771-773,
  // 8 762-767, 10 793; profiles/r03_experiments/c5_pattern_threshold.txt)
  if constexpr (!LDSM && !FUSE && !COUNT)
    if (!c->trav_frac16_global_env) kp.trav_frac16 = 8;
  if (int rs = TakeSpan(c, kp)) return rs;
  HIP_OK(hipEventRecord(c->ev[c->ev_used], c->lstream));
  hipLaunchKernelGGL((srt::sample_kernel<COUNT, LDSM, PACK, BLOCK, TEX, FUSE, GW>), dim3(blocks), dim3(BLOCK), lds, c->lstream,
                     kp);
  HIP_OK(hipGetLastError());
  HIP_OK(hipEventRecord(c->ev[c->ev_used + 1], c->lstream));
  return SRT_OK;
}

// The sphere scene (showModel false): sphere_kernel, one 256-lane block per resident slot (no stacks,
// so its LDS holds only the light records).
template <bool COUNT>
int LaunchSpheres(srt_context* c, srt::KParams kp, size_t lds) {
  int per_cu = 0;
  if (int ro = ResidentBlocks(c, &srt::sphere_kernel<COUNT>, 256, lds, &per_cu)) return ro;
  // resident blocks per CU: as many as its registers allow (C2 on one box, ms per launch: 3 blocks 3.23,
  // 4 3.00, 5 2.93; while the launch counter's atomic rate bound it, round 3, 3 were best)
  const int blocks = c->num_cus * std::min(per_cu, c->sphere_blocks);
  c->launch_per_cu = std::min(per_cu, c->sphere_blocks);
  c->launch_block = 256;
  {
    const long long waves = (long long)blocks * 4;
    const long long n_batches = (long long)kp.live_tiles * kp.nframes;
    kp.tail_start = (int)std::max<long long>(0, n_batches - (long long)c->tail_claims_sph * srt::kClaimSph * waves);
  }
  if (int rs = TakeSpan(c, kp)) return rs;
  HIP_OK(hipEventRecord(c->ev[c->ev_used], c->lstream));
  hipLaunchKernelGGL(srt::sphere_kernel<COUNT>, dim3(blocks), dim3(256), lds, c->lstream, kp);
  HIP_OK(hipGetLastError());
  HIP_OK(hipEventRecord(c->ev[c->ev_used + 1], c->lstream));
  return SRT_OK;
}

// The sample_kernel instance for the launch: counting or not, LDS-resident
// scene or global (packed stack entries when indices fit 24 bits; the timed
// global instance's schedule and waves per SIMD chosen at upload), and with
// or without the texture-sampling branch (TEX, only when a material samples).
template <bool TEX>
int LaunchMode(srt_context* c, const srt::KParams& kc, size_t lds, bool count, bool ldsm, bool pack) {
  if (!kc.show_model) return count ? LaunchSpheres<true>(c, kc, lds) : LaunchSpheres<false>(c, kc, lds);
  if (count && ldsm) return LaunchSamples<true, true, true, kLdsBlock, TEX>(c, kc, lds);
  if (count) return pack ? LaunchSamples<true, false, true, 256, TEX>(c, kc, lds)
                         : LaunchSamples<true, false, false, 256, TEX>(c, kc, lds);
  if (ldsm) return LaunchSamples<false, true, true, kLdsBlock, TEX>(c, kc, lds);
  if (c->fused && c->global_waves == 5) return pack ? LaunchSamples<false, false, true, kGw5Block, TEX, true, 5>(c, kc, lds)
                                                   : LaunchSamples<false, false, false, kGw5Block, TEX, true, 5>(c, kc, lds);
  if (c->fused) return pack ? LaunchSamples<false, false, true, 256, TEX, true>(c, kc, lds)
                            : LaunchSamples<false, false, false, 256, TEX, true>(c, kc, lds);
  return pack ? LaunchSamples<false, false, true, 256, TEX>(c, kc, lds)
              : LaunchSamples<false, false, false, 256, TEX>(c, kc, lds);
}

// pool_kernel (pool.hpp): one 1024-thread block per CU, as sample_kernel's LDS mode.
template <bool COUNT>
int LaunchPool(srt_context* c, srt::KParams kp, size_t lds) {
  const int blocks = c->num_cus;
  c->launch_per_cu = 1;
  c->launch_block = 1024;
  kp.tail_start = (int)std::max<long long>(
      0, (long long)((kp.W + 7) >> 3) * ((kp.local_rows + 7) >> 3) * kp.nframes -
             (long long)c->tail_claims * srt::kClaim * blocks * srt::kPoolTravWaves);
  HIP_OK(hipEventRecord(c->ev[c->ev_used], c->stream));
  hipLaunchKernelGGL(srt::pool_kernel<COUNT>, dim3(blocks), dim3(1024), lds, c->stream, kp);
  HIP_OK(hipGetLastError());
  HIP_OK(hipEventRecord(c->ev[c->ev_used + 1], c->stream));
  return SRT_OK;
}

// Wavefront mode (wavefront.hpp): the trace-stage kernels' instances (stack entry packing, fused
// sub-steps or the IL pattern, waves per SIMD) and their grids: as many 256-lane blocks as are resident.
template <typename F>
int Resident(srt_context* c, F* fn, size_t lds, int* blocks) {
  int per_cu = 0;
  if (int ro = ResidentBlocks(c, fn, 256, lds, &per_cu)) return ro;
  *blocks = c->num_cus * per_cu;
  return SRT_OK;
}
// The trace stage of one iteration: wf_trace_kernel, or with treelets (kp_top: the flagged node copy)
// wf_top_kernel -> wf_scan_kernel -> wf_scatter_kernel -> wf_bottom_kernel.  With `launch` false it
// only sizes the grids: *lanes = the most lanes any of them runs (their HBM stacks).
template <bool PACK, bool FUSE, int GW>
int WfStage(srt_context* c, const srt::KParams& kp, const srt::KParams& kp_top, const srt::WfParams& w, bool tl,
            bool launch, size_t* lanes) {
  const size_t ring_bytes = (size_t)256 * (PACK ? 2 : 3) * sizeof(uint32_t);
  const size_t lds = ring_bytes * (size_t)srt::global_ring(GW);
  int blocks = 0;
  if (!tl) {
    int rc = Resident(c, srt::wf_trace_kernel<PACK, FUSE, GW>, lds, &blocks);
    if (rc) return rc;
    if (lanes) *lanes = (size_t)blocks * 256;
    if (launch) {
      hipLaunchKernelGGL((srt::wf_trace_kernel<PACK, FUSE, GW>), dim3(blocks), dim3(256), lds, c->stream, kp, w);
      HIP_OK(hipGetLastError());
    }
    return SRT_OK;
  }
  const size_t lds_top = ring_bytes * (size_t)srt::kShortStack;
  int tblocks = 0;
  int rc = Resident(c, srt::wf_top_kernel<PACK, FUSE>, lds_top, &tblocks);
  if (rc) return rc;
  rc = Resident(c, srt::wf_bottom_kernel<PACK, FUSE, GW>, lds, &blocks);
  if (rc) return rc;
  if (lanes) *lanes = (size_t)std::max(blocks, tblocks) * 256;
  if (launch) {
    hipLaunchKernelGGL((srt::wf_top_kernel<PACK, FUSE>), dim3(tblocks), dim3(256), lds_top, c->stream, kp_top, w);
    hipLaunchKernelGGL(srt::wf_scan_kernel, dim3(1), dim3(1024), 0, c->stream, w);
    hipLaunchKernelGGL(srt::wf_scatter_kernel, dim3((w.slots + 255) / 256), dim3(256), 0, c->stream, w);
    hipLaunchKernelGGL((srt::wf_bottom_kernel<PACK, FUSE, GW>), dim3(blocks), dim3(256), lds, c->stream, kp, w);
    HIP_OK(hipGetLastError());
  }
  return SRT_OK;
}
template <bool PACK, bool FUSE>
int WfStageWaves(srt_context* c, const srt::KParams& kp, const srt::KParams& kt, const srt::WfParams& w, bool tl,
                 bool launch, size_t* lanes) {
  switch (c->wf_waves) {
    case 4: return WfStage<PACK, FUSE, 4>(c, kp, kt, w, tl, launch, lanes);
    case 5: return WfStage<PACK, FUSE, 5>(c, kp, kt, w, tl, launch, lanes);
    case 8: return WfStage<PACK, FUSE, 8>(c, kp, kt, w, tl, launch, lanes);
    default: return WfStage<PACK, FUSE, 6>(c, kp, kt, w, tl, launch, lanes);
  }
}
int WfTrace(srt_context* c, const srt::KParams& kp, const srt::KParams& kt, const srt::WfParams& w, bool tl,
            bool launch, size_t* lanes) {
  const bool pack = c->lds_ok;
  if (c->fused) return pack ? WfStageWaves<true, true>(c, kp, kt, w, tl, launch, lanes)
                            : WfStageWaves<false, true>(c, kp, kt, w, tl, launch, lanes);
  return pack ? WfStageWaves<true, false>(c, kp, kt, w, tl, launch, lanes)
              : WfStageWaves<false, false>(c, kp, kt, w, tl, launch, lanes);
}

// One chunk of frames through the wavefront kernels: iterations of logic -> shade -> trace over
// c->wf_slots path slots until every sample item is taken and no slot is live.  The host polls the
// live count of every 8th iteration one group late (a pinned copy and an event), so the stream stays
// full; the few iterations issued past the end find empty queues and return at once.
int LaunchWavefront(srt_context* c, srt::KParams kp, bool tex) {
  c->launch_per_cu = c->launch_block = 0;  // (its stage kernels' grids differ: no single value)
  constexpr int kMaxIters = 1 << 16;
  const uint32_t P = c->wf_slots;
  if (P > c->wf_cap) {
    FreeDev(c->d_wf_rec); FreeDev(c->d_wf_res); FreeDev(c->d_wf_state); FreeDev(c->d_wf_rayq); FreeDev(c->d_wf_hitq);
    c->d_wf_rec = nullptr; c->d_wf_res = nullptr; c->d_wf_state = c->d_wf_rayq = c->d_wf_hitq = nullptr;
    c->wf_cap = 0;
    HIP_OK(hipMalloc(&c->d_wf_rec, sizeof(float4) * 7 * (size_t)P));
    HIP_OK(hipMalloc(&c->d_wf_res, sizeof(uint2) * (size_t)P));
    HIP_OK(hipMalloc(&c->d_wf_state, sizeof(uint32_t) * (size_t)P));
    HIP_OK(hipMalloc(&c->d_wf_rayq, sizeof(uint32_t) * (size_t)P));
    HIP_OK(hipMalloc(&c->d_wf_hitq, sizeof(uint32_t) * (size_t)P));
    c->wf_cap = P;
  }
  if (!c->d_wf_ctl) {
    HIP_OK(hipMalloc(&c->d_wf_ctl, sizeof(uint32_t) * srt::WQ_WORDS * (size_t)kMaxIters));
    HIP_OK(hipMalloc(&c->d_wf_items, sizeof(uint32_t)));
    HIP_OK(hipHostMalloc(&c->h_wf_poll, 4 * sizeof(uint32_t), hipHostMallocDefault));
  }
  const long long n_items = 64LL * ((kp.W + 7) >> 3) * ((kp.local_rows + 7) >> 3) * kp.nframes;
  if (n_items >= (1LL << 31)) {  // Launch bounds the frames per chunk so this cannot happen
    srt::SetError("wavefront mode: more than 2^31 sample items in one chunk");
    return SRT_ERR_LIMIT;
  }
  HIP_OK(hipMemsetAsync(c->d_wf_state, 0, sizeof(uint32_t) * (size_t)P, c->stream));
  HIP_OK(hipMemsetAsync(c->d_wf_items, 0, sizeof(uint32_t), c->stream));
  HIP_OK(hipMemsetAsync(c->d_wf_ctl, 0, sizeof(uint32_t) * srt::WQ_WORDS * (size_t)kMaxIters, c->stream));
  srt::WfParams w;
  w.rec = c->d_wf_rec;
  w.res = c->d_wf_res;
  w.state = c->d_wf_state;
  w.rayq = c->d_wf_rayq;
  w.hitq = c->d_wf_hitq;
  w.ctl = c->d_wf_ctl;
  w.items = c->d_wf_items;
  w.slots = P;
  w.n_items = (uint32_t)n_items;
  w.iter = 0;
  kp.lights_lds = 0;  // the wavefront kernels keep no LDS copies of lights / materials
  kp.mats_lds = 0;
  const bool tl = c->n_treelets > 0 && (c->treelets >= 0 ? c->treelets == 1 : c->tl_scene);
  if (tl) {
    if (P > c->tl_cap) {
      FreeDev(c->d_tl_ray); FreeDev(c->d_tl_stk); FreeDev(c->d_tl_slist); FreeDev(c->d_tl_skey);
      FreeDev(c->d_tl_blist); FreeDev(c->d_tl_rlist);
      c->d_tl_ray = nullptr;
      c->d_tl_stk = c->d_tl_slist = c->d_tl_skey = c->d_tl_blist = c->d_tl_rlist = nullptr;
      c->tl_cap = 0;
      HIP_OK(hipMalloc(&c->d_tl_ray, sizeof(float4) * 4 * (size_t)P));
      HIP_OK(hipMalloc(&c->d_tl_stk, sizeof(uint32_t) * 3 * srt::kTopStack * (size_t)P));
      HIP_OK(hipMalloc(&c->d_tl_slist, sizeof(uint32_t) * (size_t)P));
      HIP_OK(hipMalloc(&c->d_tl_skey, sizeof(uint32_t) * (size_t)P));
      HIP_OK(hipMalloc(&c->d_tl_blist, sizeof(uint32_t) * (size_t)P));
      HIP_OK(hipMalloc(&c->d_tl_rlist, sizeof(uint32_t) * 2 * (size_t)P));
      c->tl_cap = P;
    }
    if (c->n_treelets > c->tl_count_cap) {
      FreeDev(c->d_tl_count); FreeDev(c->d_tl_fill);
      c->d_tl_count = c->d_tl_fill = nullptr;
      c->tl_count_cap = 0;
      HIP_OK(hipMalloc(&c->d_tl_count, sizeof(uint32_t) * (size_t)c->n_treelets));
      HIP_OK(hipMalloc(&c->d_tl_fill, sizeof(uint32_t) * (size_t)c->n_treelets));
      c->tl_count_cap = c->n_treelets;
    }
    HIP_OK(hipMemsetAsync(c->d_tl_count, 0, sizeof(uint32_t) * (size_t)c->n_treelets, c->stream));
    w.tray = c->d_tl_ray;
    w.tstk = c->d_tl_stk;
    w.slist = c->d_tl_slist;
    w.skey = c->d_tl_skey;
    w.blist = c->d_tl_blist;
    w.rlist[0] = c->d_tl_rlist;
    w.rlist[1] = c->d_tl_rlist + P;
    w.tcount = c->d_tl_count;
    w.tfill = c->d_tl_fill;
    w.troot = c->d_troot;
    w.n_treelets = c->n_treelets;
  } else {
    w.tray = nullptr;
    w.tstk = w.slist = w.skey = w.blist = w.rlist[0] = w.rlist[1] = w.tcount = w.tfill = nullptr;
    w.troot = nullptr;
    w.n_treelets = 0;
  }
  srt::KParams kt = kp;  // the top kernel walks the flagged node copy
  if (tl) kt.nodes = c->d_nodes_t;
  size_t lanes = 0;
  int rc = WfTrace(c, kp, kt, w, tl, false, &lanes);
  if (rc) return rc;
  {  // every trace lane's full stack in HBM, behind its LDS ring
    const size_t need = lanes * (c->lds_ok ? 2 : 3) * sizeof(uint32_t) * (size_t)kp.stack_entries;
    if (need > c->gstack_bytes) {
      FreeDev(c->d_gstack);
      c->d_gstack = nullptr;
      c->gstack_bytes = 0;
      HIP_OK(hipMalloc(&c->d_gstack, need));
      c->gstack_bytes = need;
    }
    kp.gstack = kt.gstack = c->d_gstack;
    kp.gstack_stride = kt.gstack_stride = (int)lanes;
  }
  const dim3 sgrid((P + 255) / 256);
  if (!c->wf_poll_ev[0]) {
    HIP_OK(hipEventCreateWithFlags(&c->wf_poll_ev[0], hipEventDisableTiming));
    HIP_OK(hipEventCreateWithFlags(&c->wf_poll_ev[1], hipEventDisableTiming));
  }
  hipEvent_t* poll_ev = c->wf_poll_ev;
  HIP_OK(hipEventRecord(c->ev[c->ev_used], c->stream));
  int it = 0;
  bool done = false;
  for (; it < kMaxIters && !done; ++it) {
    w.iter = it;
    hipLaunchKernelGGL(srt::wf_logic_kernel, sgrid, dim3(256), 0, c->stream, kp, w);
    if (tex) hipLaunchKernelGGL(srt::wf_shade_kernel<true>, sgrid, dim3(256), 0, c->stream, kp, w);
    else hipLaunchKernelGGL(srt::wf_shade_kernel<false>, sgrid, dim3(256), 0, c->stream, kp, w);
    HIP_OK(hipGetLastError());
    rc = WfTrace(c, kp, kt, w, tl, true, nullptr);
    if (rc) break;
    if ((it & 7) == 7) {
      const int g = (it >> 3) & 1;
      HIP_OK(hipMemcpyAsync(c->h_wf_poll + 2 * g, c->d_wf_ctl + (size_t)srt::WQ_WORDS * it + srt::WQ_LIVE,
                            sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
      HIP_OK(hipMemcpyAsync(c->h_wf_poll + 2 * g + 1, c->d_wf_items, sizeof(uint32_t), hipMemcpyDeviceToHost,
                            c->stream));
      HIP_OK(hipEventRecord(poll_ev[g], c->stream));
      if (it >= 15) {  // the previous group's poll
        HIP_OK(hipEventSynchronize(poll_ev[g ^ 1]));
        const uint32_t live = c->h_wf_poll[2 * (g ^ 1)], items = c->h_wf_poll[2 * (g ^ 1) + 1];
        done = live == 0 && (long long)items >= n_items;
      }
    }
  }
  if (rc) return rc;
  if (!done) {
    srt::SetError("wavefront mode: iteration limit reached");
    return SRT_ERR_LIMIT;
  }
  HIP_OK(hipEventRecord(c->ev[c->ev_used + 1], c->stream));
  c->wf_launched = true;
  return SRT_OK;
}

// The sky / live classification of the launch's tiles (tile_cull.hpp): recomputed on the host when something it
// reads has changed (tens of microseconds), and sent to the device -- the live tiles' list for the tile order,
// the per-tile map for accumulate_kernel -- when its result differs from the map there and the launch repays
// it.  Sending a map is not free: the copy runs on a stream of its own, the launch's streams wait for it, and
// the host waits for the last reader of the ring entry it rewrites -- measured at 0.25 ms per launch on a host
// that runs ahead of the GPU (profiles/r07_tile_cull.txt), against 19 ps saved per culled sample.  So a launch
// that would need a map other than the one on the device, and culls fewer than cull_min_samples samples
// (SRT_TILE_CULL_MIN_SAMPLES, default 2^24: about 1.3 times the break-even), runs with every tile live
// instead: a camera that moves every frame at a few spp pays the classification alone.  A context's first map
// is always sent (nothing reads the ring yet).  *use: the entry whose tiles the launch deals (nullptr: every
// tile is live).
int EnsureTileCull(srt_context* c, const srt::KParams& kp, int n_tiles, bool count, bool pool_or_wf,
                   srt_context::CullBuf** use) {
  *use = nullptr;
  std::vector<unsigned char> key;
  const auto put = [&key](const void* p, size_t n) {
    const unsigned char* b = static_cast<const unsigned char*>(p);
    key.insert(key.end(), b, b + n);
  };
  const float cam[12] = {kp.cx, kp.cy, kp.cz, kp.p00x, kp.p00y, kp.p00z, kp.dux, kp.duy, kp.duz, kp.dvx, kp.dvy, kp.dvz};
  const long long ints[14] = {kp.W, kp.H, kp.local_rows, kp.ext_w, kp.ext_h, kp.rank, kp.nranks, kp.band_rows,
                              (long long)kp.bvh_count, (long long)c->cull_gen, kp.show_model, count, pool_or_wf,
                              kp.nframes};
  put(cam, sizeof cam);
  put(ints, sizeof ints);
  // a launch too small to repay a new map even if every sample were culled is not classified either (the
  // cache is left alone, so a launch whose key it holds still uses it): every tile live
  if (key != c->cull_key && c->cull_cur >= 0 &&
      (long long)kp.W * kp.local_rows * (long long)kp.nframes < c->cull_min_samples)
    return SRT_OK;
  if (key != c->cull_key) {
    srt::TileCullIn in;
    for (int i = 0; i < 3; ++i) in.center[i] = cam[i], in.p00[i] = cam[3 + i], in.du[i] = cam[6 + i], in.dv[i] = cam[9 + i];
    in.W = kp.W;
    in.H = kp.H;
    in.local_rows = kp.local_rows;
    in.ext_w = kp.ext_w;
    in.ext_h = kp.ext_h;
    in.row_map = kp.nranks > 1 ? c->h_row_map.data() : nullptr;
    in.bvhs = c->h_bvhs.data();
    in.roots = c->h_roots.data();
    in.n_records = c->h_bvhs.size();
    in.bvh_count = kp.bvh_count;
    for (int k = 0; k < 2; ++k) in.nz_min[k] = c->nz_min[k], in.nz_max[k] = c->nz_max[k];
    in.noise_finite = c->noise_finite;
    in.show_model = kp.show_model != 0;
    in.counting = count;
    in.pool_or_wavefront = pool_or_wf;
    // (a build that ignores kp.tile_order cannot deal a list of tiles; no root boxes: nothing to test against)
    in.enabled = c->tile_cull && SRT_TILE_SCHED != 0 && c->roots_ok && c->h_roots.size() == c->h_bvhs.size() &&
                 (kp.nranks == 1 || (int)c->h_row_map.size() >= kp.local_rows);
    srt::TileCullOut out;
    srt::ClassifyTiles(in, &out);
    if ((int)out.sky.size() != n_tiles) {
      srt::SetError("tile classification and launch plan disagree on the tile count");
      return SRT_ERR_STATE;
    }
    const bool differs = out.live < n_tiles && (c->cull_cur < 0 || out.sky != c->h_tile_sky);
    if (differs && c->cull_cur >= 0 && out.culled_pixels * (long long)kp.nframes < c->cull_min_samples) {
      out.live = n_tiles;  // the launch cannot repay a new map: every tile live, the device's map stays
      out.culled_pixels = 0;
    } else if (differs) {
      const int next = (c->cull_cur + 1) % srt_context::kCullRing;
      srt_context::CullBuf& e = c->cull_ring[next];
      if (!c->cull_stream) HIP_OK(hipStreamCreateWithFlags(&c->cull_stream, hipStreamNonBlocking));
      if (!e.ready) {
        HIP_OK(hipEventCreateWithFlags(&e.ready, hipEventDisableTiming));
        HIP_OK(hipEventCreateWithFlags(&e.used, hipEventDisableTiming));
      }
      // the entry's last copy and the last launch that read it (four maps ago: long over)
      if (e.ready_rec) HIP_OK(hipEventSynchronize(e.ready));
      if (e.used_rec) HIP_OK(hipEventSynchronize(e.used));
      if (n_tiles > e.cap) {
        FreeDev(e.d_live);
        FreeDev(e.d_sky);
        if (e.h_live) (void)hipHostFree(e.h_live);
        if (e.h_sky) (void)hipHostFree(e.h_sky);
        e.d_live = e.h_live = nullptr;
        e.d_sky = e.h_sky = nullptr;
        e.cap = 0;
        HIP_OK(hipMalloc(&e.d_live, sizeof(uint32_t) * (size_t)n_tiles));
        HIP_OK(hipMalloc(&e.d_sky, (size_t)n_tiles));
        HIP_OK(hipHostMalloc(&e.h_live, sizeof(uint32_t) * (size_t)n_tiles, hipHostMallocDefault));
        HIP_OK(hipHostMalloc(&e.h_sky, (size_t)n_tiles, hipHostMallocDefault));
        e.cap = n_tiles;
      }
      int nl = 0;
      for (int t = 0; t < n_tiles; ++t) {
        e.h_sky[t] = out.sky[(size_t)t];
        if (!out.sky[(size_t)t]) e.h_live[nl++] = (uint32_t)t;
      }
      if (nl > 0) HIP_OK(hipMemcpyAsync(e.d_live, e.h_live, sizeof(uint32_t) * (size_t)nl, hipMemcpyHostToDevice, c->cull_stream));
      HIP_OK(hipMemcpyAsync(e.d_sky, e.h_sky, (size_t)n_tiles, hipMemcpyHostToDevice, c->cull_stream));
      HIP_OK(hipEventRecord(e.ready, c->cull_stream));
      e.ready_rec = true;
      e.used_rec = false;
      c->cull_cur = next;
      c->h_tile_sky = std::move(out.sky);
      ++c->cull_uploads;
    }
    c->cull_live = out.live;
    c->cull_pixels = out.culled_pixels;
    c->cull_key = std::move(key);
  }
  if (c->cull_live < n_tiles) *use = &c->cull_ring[c->cull_cur];
  return SRT_OK;
}

// Runs frames kp.frame_first .. + kp.nframes - 1 (or the reset frame) through
// sample_kernel + accumulate_kernel, in chunks that fit the sample buffer.
int Launch(srt_context* c, srt::KParams& kp, bool count) {
  const int npx = kp.local_pixels;
  if (npx <= 0) return SRT_OK;
  const dim3 pgrid((unsigned)((npx + 255) / 256));
  if (kp.reset) {
    hipLaunchKernelGGL(srt::reset_kernel, pgrid, dim3(256), 0, c->stream, kp);
    HIP_OK(hipGetLastError());
    return SRT_OK;
  }
  if (kp.nframes <= 0) return SRT_OK;
  // the launch's LDS layout and its chunks of frames (launch_plan.hpp)
  srt::LdsPlanIn in{};
  in.show_model = kp.show_model != 0;
  in.count = count;
  in.lds_ok = c->lds_ok;
  in.pairs_aligned = c->pairs_aligned;
  in.force_global = c->force_global;
  in.fused = c->fused;
  in.global_waves = c->global_waves;
  in.pool = c->pool && !c->sample_textures && kp.max_depth >= 0 && kp.max_depth <= 255;
  in.pool_slots_max = c->pool_slots_max;
  in.wavefront = c->wavefront >= 0 ? c->wavefront == 1 : c->wf_scene;
  in.nodes_lds_f4 = kp.nodes_lds_f4;
  in.tris_f4 = kp.tris_f4;
  in.stack_entries = kp.stack_entries;
  in.light_records = kp.light_records;
  in.n_mats = c->n_mats;
  in.has_mats = c->d_mats != nullptr;
  in.top_f4 = c->top_f4;
  const srt::LdsPlan plan = srt::PlanLds(kBuild, in);
  const bool ldsm = plan.ldsm, pool = plan.pool, wf = plan.wf;
  const size_t lds = plan.lds;
  kp.stack_base_f4 = plan.stack_base_f4;
  kp.coop_off = plan.coop_off;
  kp.top_f4 = plan.top_f4;
  kp.top_lds_f4 = plan.top_lds_f4;
  kp.lights_lds = plan.lights_lds;
  kp.lights_base_f4 = plan.lights_base_f4;
  kp.mats_lds = plan.mats_lds;
  kp.mat_records = plan.mat_records;
  kp.mats_base_f4 = plan.mats_base_f4;
  if (!ldsm && kp.show_model) c->launch_top_f4 = plan.top_f4;  // (of the last global-scene launch)
  c->launch_mats_lds = plan.mats_lds;
  if (pool) {
    kp.pool_ctl_off = plan.pool_ctl_off;
    kp.pool_ring_off = plan.pool_ring_off;
    kp.pool_rec_off = plan.pool_rec_off;
    kp.pool_cap = plan.pool_cap;
    kp.pool_slots = plan.pool_slots;
    kp.pool_batch = c->pool_batch;
    kp.pool_tlow = c->pool_tlow;
    kp.pool_deadline = (unsigned long long)c->pool_deadline_ms * 100000ull;  // s_memrealtime runs at 100 MHz
  }
  const srt::ChunkPlan chunks = srt::PlanChunks(kp.W, kp.local_rows, npx, kp.nframes, wf, c->lbuf_total, c->pipe);
  const size_t n_tiles = chunks.n_tiles, need = chunks.need;
  const int chunk = chunks.chunk, nchunks = chunks.nchunks;
  const bool piped = !count && !pool && !wf && c->pipe > 1;
  // timed sample_kernel launches of a mesh scene deal only the tiles that are not provably sky; counting
  // launches keep every tile (their counts stay the reference's), as do the sphere scene, pool and wavefront mode
  srt_context::CullBuf* cullbuf = nullptr;
  if (int rt = EnsureTileCull(c, kp, (int)n_tiles, count, pool || wf, &cullbuf)) return rt;
  const bool cull = cullbuf != nullptr;
  const int n_live = cull ? c->cull_live : (int)n_tiles;
  const uint32_t* live_list = cull ? cullbuf->d_live : nullptr;
  c->launch_live_tiles = n_live;
  c->launch_culled = cull ? c->cull_pixels * (long long)kp.nframes : 0;
  // (a counting launch, the untimed first launch of a measurement, sets the slots up for the timed ones)
  if ((piped || (count && c->pipe > 1)) && c->slots.empty()) {
    c->slots.resize((size_t)c->pipe);
    for (auto& sl : c->slots) {
      HIP_OK(hipStreamCreateWithFlags(&sl.stream, hipStreamNonBlocking));
      HIP_OK(hipEventCreateWithFlags(&sl.sampled, hipEventDisableTiming));
      HIP_OK(hipEventCreateWithFlags(&sl.accumulated, hipEventDisableTiming));
    }
  }
  kp.trav_frac16 = ldsm ? c->trav_frac16 : c->trav_frac16_global;
  kp.bounce_cap = c->bounce_cap;
  // (ST_POOLERR, the last entry, is sticky: a watchdog that fired in an earlier launch of this
  // render must still reach srt_finish, which reads and clears it)
  static_assert(srt::ST_POOLERR + 1 == srt::ST_TOTAL, "ST_POOLERR must stay the last stats entry");
  HIP_OK(hipMemsetAsync(c->d_stats, 0, sizeof(unsigned long long) * srt::ST_POOLERR, c->stream));
  const int out_frames = kp.frame_first + kp.nframes - 1;
  while ((int)c->ev.size() < 2 * nchunks) {
    hipEvent_t e;
    HIP_OK(hipEventCreate(&e));
    c->ev.push_back(e);
  }
  c->ev_used = 0;
  c->chunk_span.assign((size_t)nchunks, -1);
  // The launch buffers: the context's own on `stream`, or (piped) one slot's per chunk on the slot's
  // stream.  A piped chunk's batch counter is the slot's one word (its previous launch is accumulated).
  const int ctr_need = piped ? 1 : nchunks;
  const bool overlap = c->pipe_overlap == 2 || (c->pipe_overlap == 1 && c->nranks > 1);
  c->launch_overlap = piped && overlap;
  if (piped || (count && c->pipe > 1)) {  // every slot's sample buffer now: a timed loop allocates none
    for (auto& sl : c->slots) {
      if (sl.lbuf_bytes >= need) continue;
      if (sl.pending) HIP_OK(hipEventSynchronize(sl.accumulated));
      FreeDev(sl.lbuf);
      sl.lbuf = nullptr;
      sl.lbuf_bytes = 0;
      HIP_OK(hipMalloc(&sl.lbuf, need));
      sl.lbuf_bytes = need;
    }
  }
  for (int f0 = 0; f0 < kp.nframes; f0 += chunk) {
    srt_context::Slot* sl = piped ? &c->slots[(size_t)(c->pipe_seq++ % (unsigned long long)c->pipe)] : nullptr;
    if (sl) {
      if (sl->pending) HIP_OK(hipStreamWaitEvent(sl->stream, sl->accumulated, 0));
      if (!overlap && c->last_sampled) HIP_OK(hipStreamWaitEvent(sl->stream, c->last_sampled, 0));
      SwapSlot(c, *sl, overlap);
      c->lstream = sl->stream;
      c->lidle = sl->pending ? sl->accumulated : nullptr;
      c->lidle2 = overlap ? nullptr : c->last_sampled;
    }
    if (!sl) {  // launches in series may still read the shared stacks and tile arrays
      c->lidle = nullptr;
      c->lidle2 = c->last_sampled;
    }
    const hipStream_t ls = c->lstream;
    int rc = SRT_OK;
    do {  // (one pass: `break` on an error, so the slot's buffers are swapped back)
      const bool grow = need > c->lbuf_bytes || ctr_need > c->batch_ctr_cap || (int)n_tiles > c->tile_cap;
      if (grow && WaitLaunchIdle(c) != SRT_OK) { rc = SRT_ERR_HIP; break; }  // earlier launches still read them
      if (need > c->lbuf_bytes) {
        FreeDev(c->d_lbuf);
        c->d_lbuf = nullptr;
        c->lbuf_bytes = 0;
        if (hipMalloc(&c->d_lbuf, need) != hipSuccess) { srt::SetError("hipMalloc(sample buffer) failed"); rc = SRT_ERR_HIP; break; }
        c->lbuf_bytes = need;
      }
      if (ctr_need > c->batch_ctr_cap) {
        FreeDev(c->d_batch_ctr);
        c->d_batch_ctr = nullptr;
        c->batch_ctr_cap = 0;
        if (hipMalloc(&c->d_batch_ctr, sizeof(unsigned long long) * (size_t)ctr_need) != hipSuccess) {
          srt::SetError("hipMalloc(batch counters) failed");
          rc = SRT_ERR_HIP;
          break;
        }
        c->batch_ctr_cap = ctr_need;
      }
      if (!sl && f0 == 0)
        if (hipMemsetAsync(c->d_batch_ctr, 0, sizeof(unsigned long long) * (size_t)nchunks, ls) != hipSuccess) { rc = HipFail("sample launch"); break; }
      if (sl && hipMemsetAsync(c->d_batch_ctr, 0, sizeof(unsigned long long), ls) != hipSuccess) { rc = HipFail("sample launch"); break; }
      srt::KParams kc = kp;
      kc.lbuf = c->d_lbuf;
      kc.frame_first = kp.frame_first + f0;
      kc.nframes = std::min(chunk, kp.nframes - f0);
      kc.write_output = (f0 + chunk >= kp.nframes) ? kp.write_output : 0;
      kc.batch_ctr = reinterpret_cast<uint32_t*>(c->d_batch_ctr + (sl ? 0 : f0 / chunk));
      {  // tile order: the tiles the last launch found most expensive first (SRT_TILE_ORDER=0: natural order)
        const int nt = (int)n_tiles;
        if (nt > c->tile_cap) {
          FreeDev(c->d_tile_cost);
          FreeDev(c->d_tile_order);
          c->d_tile_cost = c->d_tile_order = nullptr;
          c->tile_cap = 0;
          if (hipMalloc(&c->d_tile_cost, sizeof(uint32_t) * (size_t)nt) != hipSuccess ||
              hipMalloc(&c->d_tile_order, sizeof(uint32_t) * (size_t)nt) != hipSuccess) {
            srt::SetError("hipMalloc(tile order) failed");
            rc = SRT_ERR_HIP;
            break;
          }
          c->tile_cap = nt;
          c->tile_costs_for = -1;
        }
        // the live tiles' list and the sky map may still be on their way (EnsureTileCull)
        if (cull && hipStreamWaitEvent(ls, cullbuf->ready, 0) != hipSuccess) { rc = HipFail("sample launch"); break; }
        if (cull && ls != c->stream && hipStreamWaitEvent(c->stream, cullbuf->ready, 0) != hipSuccess) { rc = HipFail("sample launch"); break; }
        // (the costs are kept per tile, so they stay good when the live set changes; a sky tile's is neither
        // read nor written, so a tile that turns live again is placed by the cost its last live launch left:
        // that only moves it in the schedule)
        if (c->tile_schedule && c->tile_costs_for == nt) {
          if (n_live > 0)
            hipLaunchKernelGGL(srt::order_tiles_kernel, dim3(1), dim3(1024), 0, ls, c->d_tile_cost, c->d_tile_order,
                               live_list, n_live);
        } else {
          if (n_live > 0)
            hipLaunchKernelGGL(srt::iota_kernel, dim3((n_live + 255) / 256), dim3(256), 0, ls, c->d_tile_order, live_list,
                               n_live);
          if (c->tile_schedule && hipMemsetAsync(c->d_tile_cost, 0, sizeof(uint32_t) * (size_t)nt, ls) != hipSuccess) {
            rc = HipFail("sample launch");
            break;
          }
        }
        if (hipGetLastError() != hipSuccess) { rc = HipFail("sample launch"); break; }
        kc.tile_order = c->d_tile_order;
        kc.live_tiles = n_live;
        kc.tile_sky = cull ? cullbuf->d_sky : nullptr;
        kc.tile_cost = c->tile_schedule ? c->d_tile_cost : nullptr;
        c->tile_costs_for = c->tile_schedule ? nt : -1;
      }
      // LDS mode: packed entries (lds_ok); global-scene mode: packed when indices fit 24 bits
      const bool pack = c->lds_ok;
      if (pool) rc = count ? LaunchPool<true>(c, kc, lds) : LaunchPool<false>(c, kc, lds);
      else if (wf) rc = LaunchWavefront(c, kc, c->sample_textures);
      else rc = c->sample_textures ? LaunchMode<true>(c, kc, lds, count, ldsm, pack)
                                   : LaunchMode<false>(c, kc, lds, count, ldsm, pack);
      if (rc) break;
      c->pool_launched |= pool;
      c->ev_used += 2;  // LaunchSamples recorded the pair around the launch
      if (!sl) {  // a later launch in series (sharing the tile order) waits for this one
        if (!c->plain_done && hipEventCreateWithFlags(&c->plain_done, hipEventDisableTiming) != hipSuccess) {
          rc = HipFail("sample launch");
          break;
        }
        if (hipEventRecord(c->plain_done, c->stream) != hipSuccess) { rc = HipFail("sample launch"); break; }
        c->last_sampled = c->plain_done;
      }
      if (sl) {  // the accumulation follows the samples on `stream`
        c->last_sampled = sl->sampled;
        if (hipEventRecord(sl->sampled, ls) != hipSuccess || hipStreamWaitEvent(c->stream, sl->sampled, 0) != hipSuccess) {
          rc = HipFail("sample launch");
          break;
        }
      }
      hipLaunchKernelGGL(srt::accumulate_kernel, pgrid, dim3(256), 0, c->stream, kc, out_frames);
      if (hipGetLastError() != hipSuccess) { rc = HipFail("sample launch"); break; }
      if (cull) {  // the map's entry may be rewritten once this launch's kernels have read it
        if (hipEventRecord(cullbuf->used, c->stream) != hipSuccess) { rc = HipFail("sample launch"); break; }
        cullbuf->used_rec = true;
      }
      if (sl) {
        if (hipEventRecord(sl->accumulated, c->stream) != hipSuccess) { rc = HipFail("sample launch"); break; }
        sl->pending = true;
      }
    } while (false);
    if (sl) {
      SwapSlot(c, *sl, overlap);
      c->lstream = c->stream;
    }
    c->lidle = c->lidle2 = nullptr;
    if (rc) return rc;
  }
  if (count) {
    unsigned long long s[srt::ST_N];
    HIP_OK(hipMemcpyAsync(s, c->d_stats, sizeof(s), hipMemcpyDeviceToHost, c->stream));
    HIP_OK(hipStreamSynchronize(c->stream));
    c->stats.rays += s[srt::ST_RAYS];
    c->stats.nodes += s[srt::ST_NODES];
    c->stats.tris += s[srt::ST_TRIS];
    c->stats.rng_u += s[srt::ST_RNGU];
    c->stats.rng_sq += s[srt::ST_RNGSQ];
    c->stats.light_reads += s[srt::ST_LIGHTS];
    c->stats.mat_reads += s[srt::ST_MATS];
    c->stats.samples += s[srt::ST_SAMPLES];
    c->stats.stack_overflow += s[srt::ST_OVERFLOW];
    c->stats.bounce_cap += s[srt::ST_BOUNCECAP];
    c->stats.max_stack = std::max<uint64_t>(c->stats.max_stack, s[srt::ST_MAXSTACK]);
    c->shadow_rays += s[srt::ST_SHADOW];
  }
  return SRT_OK;
}

// One array of a scene image onto the device (`*dst` stays null for an empty one); the caller synchronizes.
template <typename T>
int UploadArray(srt_context* c, T** dst, const std::vector<T>& src) {
  if (src.empty()) return SRT_OK;
  HIP_OK(hipMalloc(dst, src.size() * sizeof(T)));
  HIP_OK(hipMemcpyAsync(*dst, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice, c->stream));
  return SRT_OK;
}

}  // namespace

namespace srt {

// The multi-GPU root's assembly kernels on a given stream (srt_assemble_bands /
// srt_assemble_output_bands use the context's own; the device group its gather stream).
int AssembleBandsOn(srt_context* c, void* stream, const void* gathered, int nranks, int rows_pad, int band_rows,
                    int frames, void* accum_full, void* out_full) {
  if (!c || !gathered || nranks < 1 || rows_pad < 1 || band_rows < 1 || frames < 1 || c->W <= 0 || c->H <= 0)
    return SRT_ERR_INVALID;
  HIP_OK(hipSetDevice(c->device));
  const size_t n = (size_t)c->W * (size_t)c->H;
  hipLaunchKernelGGL(srt::assemble_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), static_cast<const float4*>(gathered), nranks, rows_pad, c->W,
                     c->H, band_rows, frames, static_cast<float4*>(accum_full), static_cast<uint32_t*>(out_full));
  HIP_OK(hipGetLastError());
  return SRT_OK;
}

int AssembleOutputOn(srt_context* c, void* stream, const void* gathered_rgba8, int nranks, int rows_pad,
                     int band_rows, int ext_w, int ext_h, void* out_full) {
  if (!c || !gathered_rgba8 || !out_full || nranks < 1 || rows_pad < 1 || band_rows < 1 || c->W <= 0 || c->H <= 0)
    return SRT_ERR_INVALID;
  HIP_OK(hipSetDevice(c->device));
  const size_t n = (size_t)c->W * (size_t)c->H;
  hipLaunchKernelGGL(srt::assemble_out_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), static_cast<const uint32_t*>(gathered_rgba8), nranks, rows_pad,
                     c->W, c->H, band_rows, std::min(ext_w, c->W), std::min(ext_h, c->H),
                     static_cast<uint32_t*>(out_full));
  HIP_OK(hipGetLastError());
  return SRT_OK;
}

}  // namespace srt

// ===========================================================================
// C ABI (launch part; context.cpp holds the rest)
// ===========================================================================
extern "C" {

#ifndef SRT_CODE_HASH
#define SRT_CODE_HASH "unknown"
#endif
const char* srt_code_hash(void) { return SRT_CODE_HASH; }

int srt_dispatch(srt_context* c, uint32_t gx, uint32_t gy) {
  if (!c) return SRT_ERR_INVALID;
  HIP_OK(hipSetDevice(c->device));
  srt::KParams kp;
  int rc = FillParams(c, &kp, true);
  if (rc) return rc;
  kp.ext_w = (int)std::min<uint64_t>((uint64_t)gx * 8, (uint64_t)c->W);
  kp.ext_h = (int)std::min<uint64_t>((uint64_t)gy * 8, (uint64_t)c->H);
  kp.frame_first = c->accum_frames;
  kp.nframes = 1;
  kp.write_output = 1;
  kp.reset = c->reset;
  if (!kp.reset && c->accum_frames == 0) {
    srt::SetError("accumFrames must be >= 1 for a sampling dispatch (the reference increments it first)");
    return SRT_ERR_STATE;
  }
  return Launch(c, kp, false);
}

int srt_render_frames(srt_context* c, int frame_first, int nframes, int write_output, int count) {
  if (!c || nframes < 0 || frame_first < 1) return SRT_ERR_INVALID;
  HIP_OK(hipSetDevice(c->device));
  srt::KParams kp;
  int rc = FillParams(c, &kp, true);
  if (rc) return rc;
  if (nframes == 0) return SRT_OK;
  kp.frame_first = frame_first;
  kp.nframes = nframes;
  kp.write_output = write_output ? 1 : 0;
  kp.reset = 0;
  rc = Launch(c, kp, count != 0);
  if (rc == SRT_OK) c->accum_frames = frame_first + nframes - 1;  // the uniform as the last dispatch leaves it
  return rc;
}

int srt_finish(srt_context* c) {
  if (!c) return SRT_ERR_INVALID;
  HIP_OK(hipStreamSynchronize(c->stream));
  if (c->pool_launched) {  // pool_kernel's watchdog (pool.hpp): a launch that overran its deadline
    unsigned long long err = 0;
    HIP_OK(hipMemcpy(&err, c->d_stats + srt::ST_POOLERR, sizeof(err), hipMemcpyDeviceToHost));
    HIP_OK(hipMemset(c->d_stats + srt::ST_POOLERR, 0, sizeof(err)));
    c->pool_launched = false;
    if (err) {
      srt::SetError("pool_kernel: watchdog expired (the render is incomplete)");
      return SRT_ERR_HIP;
    }
  }
  return SRT_OK;
}

// Diagnostic: shader-clock cycles per phase of the last render (SRT_PHASE_TIMING builds only; zeros otherwise).
// out[0..3]: refill / traversal / shading cycles, outer iterations; out[4..9]: traversal
// iterations and summed lane counts (working, traversing, at a leaf, at an internal node),
// lanes shading (summed over outer iterations).
// out[10..57]: per sub-step k (3 values): lanes taking it, waves executing it, lanes popping after it.
extern "C" int srt_debug_phase_cycles(srt_context* c, unsigned long long out[58]) {
  if (!c || !out) return SRT_ERR_INVALID;
  HIP_OK(hipMemcpyAsync(out, c->d_stats + srt::ST_CYC_REFILL, 58 * sizeof(unsigned long long), hipMemcpyDeviceToHost,
                        c->stream));
  HIP_OK(hipStreamSynchronize(c->stream));
  return SRT_OK;
}

#ifdef SRT_WAVE_TRACE
// Diagnostic build: copies the last launch's per-wave stamps (start, scene in
// LDS, batches exhausted, end; s_memrealtime ticks) into out[4 * n], n <= waves.
extern "C" int srt_debug_wave_trace(srt_context* c, unsigned long long* out, int n) {
  if (!c || !out || !c->d_trace) return -1;
  n = std::min(n, c->trace_waves);
  HIP_OK(hipMemcpyAsync(out, c->d_trace, (size_t)n * 4 * sizeof(unsigned long long), hipMemcpyDeviceToHost,
                        c->stream));
  HIP_OK(hipStreamSynchronize(c->stream));
  return n;
}
#endif

int srt_upload_scene(srt_context* c, const srt_bvh_record* bvhs, uint32_t n_bvhs, const srt_bvh_node* nodes,
                     uint32_t n_nodes, const srt_material_obj* mats, const float* tex_albedo, uint32_t n_mats,
                     const srt_triangle* tris, uint32_t n_tris, const srt_vertex* verts, uint32_t n_verts) {
  if (!c || (n_bvhs && !bvhs) || (n_nodes && !nodes) || (n_mats && !mats) || (n_tris && !tris) ||
      (n_verts && !verts))
    return SRT_ERR_INVALID;
  if (int rq = Quiesce(c)) return rq;  // pipelined launches still read the old scene
  if (n_nodes == 0 || n_bvhs == 0) {
    srt::SetError("scene needs at least one BVH and one node");
    return SRT_ERR_INVALID;
  }
  int depth = 0;
  std::vector<std::pair<uint32_t, uint32_t>> tri_ranges;
  std::vector<uint8_t> reach;
  int rc = ValidateNodes(nodes, n_nodes, n_tris, bvhs, n_bvhs, &depth, &tri_ranges, &reach);
  if (rc) return rc;
  HIP_OK(hipSetDevice(c->device));
  // what the scene's size chooses, and the arrays and scalars of the device layout (scene_image.hpp)
  const srt::ScenePolicy policy = srt::ChooseScenePolicy(n_nodes, n_tris, c->treelet_depth, c->treelets);
  const srt::SceneArrays in{bvhs, n_bvhs, nodes, n_nodes, mats, tex_albedo, n_mats, tris, n_tris, verts, n_verts};
  srt::SceneImage img;
  srt::BuildSceneImage(in, depth, std::move(tri_ranges), reach, policy, kBuild, c->h_lights.size(), &img);
  c->global_waves = policy.global_waves;
  c->tl_scene = policy.tl_scene;
  FreeDev(c->d_nodes_t);
  FreeDev(c->d_troot);
  c->d_nodes_t = nullptr;
  c->d_troot = nullptr;
  c->n_treelets = 0;
  if ((rc = UploadArray(c, &c->d_nodes_t, img.nodes_t))) return rc;
  if ((rc = UploadArray(c, &c->d_troot, img.troot))) return rc;
  if (!img.troot.empty()) HIP_OK(hipStreamSynchronize(c->stream));
  c->n_treelets = (uint32_t)img.troot.size();
  FreeDev(c->d_nodes); FreeDev(c->d_mats); FreeDev(c->d_tris); FreeDev(c->d_tri_uv);
  c->d_nodes = nullptr; c->d_mats = nullptr; c->d_tris = nullptr; c->d_tri_uv = nullptr;
  c->scene_ok = false;
  if ((rc = UploadArray(c, &c->d_tri_uv, img.tri_uv))) return rc;
  if ((rc = UploadArray(c, &c->d_nodes, img.nodes))) return rc;
  if ((rc = UploadArray(c, &c->d_mats, img.mats))) return rc;
  if ((rc = UploadArray(c, &c->d_tris, img.tris))) return rc;
  HIP_OK(hipStreamSynchronize(c->stream));
  c->h_bvhs = std::move(img.bvhs);
  c->h_roots.assign(c->h_bvhs.size(), srt::RootBox{});  // each record's root box, as the kernels read it (tile_cull.hpp)
  c->roots_ok = true;
  for (size_t i = 0; i < c->h_bvhs.size(); ++i) {
    const size_t at = 2 * (size_t)c->h_bvhs[i].first_index + 2;
    if (at + 2 > img.nodes.size()) {  // no box to read: culling stays off for this scene (EnsureTileCull)
      c->roots_ok = false;
      break;
    }
    const float4 lo = img.nodes[at], hi = img.nodes[at + 1];
    c->h_roots[i] = srt::RootBox{{lo.x, lo.y, lo.z}, {hi.x, hi.y, hi.z}};
  }
  ++c->cull_gen;
  c->bvh_tris = std::move(img.bvh_tris);
  c->sample_textures = img.sampled;
  c->bvhs_dirty = true;
  c->n_nodes = img.n_slots + srt::kNodePad;
  c->top_f4 = img.n_top > 0 ? 2 * (int)img.n_top + 2 : 0;  // float4 of slots [0, n_top)
  c->top_depth = img.top_depth;
  c->ref_or = img.ref_or;
  c->n_tris = img.n_tslots;  // device records (slots)
  c->n_mats = n_mats;
  c->stack_entries = img.depth + 1;
  c->lds_ok = img.lds_ok;
  c->fused = img.fused;
  c->pairs_aligned = img.pairs_aligned;
  c->scene_ok = true;
  if (c->bvh_count == 0) c->bvh_count = n_bvhs;
  // the zero records beyond n_bvhs traverse from node 0 with a zero ray
  // (raytrace_compute.glsl:144-147 reading bvhs[i] out of bounds)
  return SRT_OK;
}

int srt_upload_textures(srt_context* c, const srt_texture* textures, uint32_t n) {
  if (!c || (n && !textures)) return SRT_ERR_INVALID;
  if (int rq = Quiesce(c)) return rq;
  std::vector<uint4> info(std::max<uint32_t>(n, 1), make_uint4(0, 0, 0, 0));
  size_t total = 0;
  for (uint32_t i = 0; i < n; ++i) {
    const srt_texture& t = textures[i];
    if (!t.texels || t.width <= 0 || t.height <= 0 || t.channels < 1 || t.channels > 4) {
      srt::SetError("texture " + std::to_string(i) + ": bad size, channel count or texel pointer");
      return SRT_ERR_INVALID;
    }
    info[i] = make_uint4((uint32_t)total, (uint32_t)t.width, (uint32_t)t.height, 0u);
    total += (size_t)t.width * (size_t)t.height;
    if (total >= (1ull << 32)) {
      srt::SetError("textures hold more than 2^32 texels");
      return SRT_ERR_LIMIT;
    }
  }
  // GL_RED reads (r, 0, 0), a 2-channel file (r, g, 0); channel values are c / 255 (unorm8)
#if SRT_TEX8
  // the file's bytes, RGBA8 (the kernel's unorm8 reads c / 255 exactly): 4 B a texel
  using Texel = uint32_t;
  std::vector<Texel> tx(std::max<size_t>(total, 1), 0u);
#else
  using Texel = float4;  // RGBA32F, c / 255
  std::vector<Texel> tx(std::max<size_t>(total, 1), make_float4(0, 0, 0, 0));
#endif
  for (uint32_t i = 0; i < n; ++i) {
    const srt_texture& t = textures[i];
    const size_t m = (size_t)t.width * (size_t)t.height;
    for (size_t k = 0; k < m; ++k) {
      const uint8_t* p = t.texels + k * t.channels;
      uint32_t v[3] = {0u, 0u, 0u};
      for (int ch = 0; ch < t.channels && ch < 3; ++ch) v[ch] = p[ch];
      if (t.channels == 2) v[2] = 0u;
#if SRT_TEX8
      tx[info[i].x + k] = v[0] | (v[1] << 8) | (v[2] << 16);
#else
      tx[info[i].x + k] = make_float4((float)v[0] / 255.0f, (float)v[1] / 255.0f, (float)v[2] / 255.0f, 1.0f);
#endif
    }
  }
  HIP_OK(hipSetDevice(c->device));
  FreeDev(c->d_tex); FreeDev(c->d_tex_info);
  c->d_tex = nullptr; c->d_tex_info = nullptr; c->n_tex = 0;
  HIP_OK(hipMalloc(&c->d_tex, tx.size() * sizeof(Texel)));
  HIP_OK(hipMalloc(&c->d_tex_info, info.size() * sizeof(uint4)));
  HIP_OK(hipMemcpyAsync(c->d_tex, tx.data(), tx.size() * sizeof(Texel), hipMemcpyHostToDevice, c->stream));
  HIP_OK(hipMemcpyAsync(c->d_tex_info, info.data(), info.size() * sizeof(uint4), hipMemcpyHostToDevice, c->stream));
  HIP_OK(hipStreamSynchronize(c->stream));
  c->n_tex = n;
  return SRT_OK;
}

int srt_update_model_matrix(srt_context* c, uint32_t index, const float frame[16]) {
  if (!c || !frame) return SRT_ERR_INVALID;
  if (index >= c->h_bvhs.size()) {
    srt::SetError("UpdateModelMatrix: index out of range");  // std::vector::at throws
    return SRT_ERR_INVALID;
  }
  std::memcpy(c->h_bvhs[index].frame, frame, sizeof(float) * 16);
  c->bvhs_dirty = true;
  ++c->cull_gen;
  return SRT_OK;  // pushed to the device at the next launch (EnsureBvhs)
}

int srt_trace_closest(srt_context* c, const srt_ray* rays, uint32_t n, uint32_t* hits, float* t_out) {
  if (!c || (n && (!rays || !hits || !t_out))) return SRT_ERR_INVALID;
  if (!c->scene_ok) { srt::SetError("no scene uploaded"); return SRT_ERR_STATE; }
  if (n == 0) return SRT_OK;
  HIP_OK(hipSetDevice(c->device));
  srt::KParams kp;
  std::memset(&kp, 0, sizeof kp);
  int rc = EnsureBvhs(c);
  if (rc) return rc;
  kp.nodes = c->d_nodes;
  kp.ref_or = c->ref_or;
  kp.tris = c->d_tris;
  kp.bvhs = c->d_bvhs;
  kp.bvh_count = c->bvh_count;
  kp.stack_entries = c->stack_entries;
  kp.stats = c->d_stats;
  // one 3-dword stack entry per tree level and lane: in LDS while 64 KiB hold a 256- (down to 64-)
  // lane block's stacks, else in HBM (lane-interleaved; trees deeper than ~85 levels)
  const size_t entry = 3 * sizeof(uint32_t) * (size_t)kp.stack_entries;
  int block = 256;
  while (block > 64 && (size_t)block * entry > 65536) block >>= 1;
  const bool hbm_stack = (size_t)block * entry > 65536;
  const size_t lds = hbm_stack ? 0 : (size_t)block * entry;
  // device buffers, freed on every path
  struct Buf {
    void* p = nullptr;
    ~Buf() { if (p) (void)hipFree(p); }
  } d_rays, d_hits, d_t, d_stk;
  HIP_OK(hipMalloc(&d_rays.p, sizeof(srt_ray) * n));
  HIP_OK(hipMalloc(&d_hits.p, sizeof(uint32_t) * n));
  HIP_OK(hipMalloc(&d_t.p, sizeof(float) * n));
  const size_t grid = (n + block - 1) / block;
  if (hbm_stack) HIP_OK(hipMalloc(&d_stk.p, entry * grid * (size_t)block));  // one area per block
  HIP_OK(hipMemcpyAsync(d_rays.p, rays, sizeof(srt_ray) * n, hipMemcpyHostToDevice, c->stream));
  HIP_OK(hipMemsetAsync(c->d_stats, 0, sizeof(unsigned long long) * srt::ST_N, c->stream));
  hipLaunchKernelGGL(srt::closest_kernel, dim3((unsigned)grid), dim3(block), lds, c->stream, kp,
                     static_cast<const srt_ray*>(d_rays.p), n, static_cast<uint32_t*>(d_hits.p),
                     static_cast<float*>(d_t.p), static_cast<uint32_t*>(d_stk.p));
  HIP_OK(hipGetLastError());
  unsigned long long s[srt::ST_N];
  HIP_OK(hipMemcpyAsync(hits, d_hits.p, sizeof(uint32_t) * n, hipMemcpyDeviceToHost, c->stream));
  HIP_OK(hipMemcpyAsync(t_out, d_t.p, sizeof(float) * n, hipMemcpyDeviceToHost, c->stream));
  HIP_OK(hipMemcpyAsync(s, c->d_stats, sizeof(s), hipMemcpyDeviceToHost, c->stream));
  HIP_OK(hipStreamSynchronize(c->stream));
  c->stats.rays += n;
  c->stats.nodes += s[srt::ST_NODES];
  c->stats.tris += s[srt::ST_TRIS];
  return SRT_OK;
}

}  // extern "C"
