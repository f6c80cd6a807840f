// launch_plan.cpp -- see launch_plan.hpp.
#include "launch_plan.hpp"

namespace srt {

namespace {

// One layout: pool mode's (`pool`, LDS mode only) or sample_kernel's / sphere_kernel's.  A pool layout
// without room for 64 records comes back with pool_slots == 0.
LdsPlan Layout(const BuildConsts& k, const LdsPlanIn& in, bool ldsm, bool pool) {
  LdsPlan p{};
  p.ldsm = ldsm;
  p.pool = pool;
  p.gw = (!in.count && in.fused) ? in.global_waves : 4;  // global-scene mode: LaunchMode's instance
  p.block = ldsm ? k.lds_block : GlobalBlock(k, !in.count && in.fused, p.gw);
  p.wf = !ldsm && !in.count && in.show_model && in.wavefront;
  const size_t scene_bytes = ((size_t)in.nodes_lds_f4 + (size_t)in.tris_f4) * kF4;
  size_t lds = 0;
  if (ldsm) {  // the scene, then 2-dword stacks: every lane's, or (pool.hpp) the traversal waves' only
    p.stack_base_f4 = in.nodes_lds_f4 + in.tris_f4;
    lds = scene_bytes + (size_t)(pool ? k.pool_trav_lanes : k.lds_block) * 2 * sizeof(uint32_t) * (size_t)in.stack_entries;
  } else if (in.show_model) {  // LDS rings of global_ring(waves) entries per lane, backed by HBM stacks
    lds = RingBytes(k, p.block, in.lds_ok, p.gw);
    if (k.coop && !in.count && in.fused) {  // the fused sub-steps' load stages, one per wave
      lds = Align16(lds);
      p.coop_off = (int)lds;
      lds += (size_t)(p.block / 64) * k.coop_wave_bytes;
    }
    // the top levels' pairs (LayoutNodes' first region) for the fused instance, when they fit beside the
    // rings and this launch's light records (placed behind it, below) within the LDS one of the
    // instance's blocks may take; the material records follow only if they still fit that share, else
    // shading reads them from HBM, so neither costs a resident block per CU, and the region,
    // worth ~10% on a surface mesh, is never given up for them; wavefront mode's kernels read none.
    // (TopRegionBudget, launch_plan.hpp, is what the upload sized the region with.)
    if (!in.count && in.fused && !in.wavefront && in.top_f4 > 0) {
      lds = Align16(lds);
      const size_t tb = TopRegionBytes(k, (size_t)in.top_f4);
      if (lds + tb + LightLdsBytes((size_t)in.light_records) <= GlobalBlockLds(p.block, p.gw)) {
        p.top_f4 = in.top_f4;
        p.top_lds_f4 = (int)(lds / kF4);
        lds += tb;
      }
    }
  }  // (else the sphere scene, sphere_kernel: no traversal stacks)
  // light and material records in LDS behind the rest, when they fit (shading reads them there) within
  // the LDS one block may take: all of it in LDS mode, a global-scene block's share at its instance's
  // blocks per CU (records past it would cost a resident block per CU; they are read from HBM instead)
  const size_t cap = (!ldsm && in.show_model) ? GlobalBlockLds(p.block, p.gw) : kLdsBytes;
  lds = Align16(lds);
  const size_t light_bytes = 2 * kF4 * ((size_t)in.light_records + 1);
  p.lights_lds = (LightLdsBytes((size_t)in.light_records) != 0 && lds + light_bytes <= cap) ? 1 : 0;
  if (p.lights_lds) {
    p.lights_base_f4 = (int)(lds / kF4);
    lds += light_bytes;
  }
  p.mat_records = (int)in.n_mats + 1;
  const size_t mat_bytes = 2 * kF4 * (size_t)p.mat_records;
  p.mats_lds = (in.show_model && in.has_mats && mat_bytes <= 16384 && lds + mat_bytes <= cap) ? 1 : 0;
  if (p.mats_lds) {
    p.mats_base_f4 = (int)(lds / kF4);
    lds += mat_bytes;
  }
  if (pool) {  // control words, 3 rings of u32 record ids (power-of-two capacity), 112-B records
    const size_t ctl = lds;
    lds += 16 * sizeof(uint32_t);
    int slots = 0, ring = 1;
    for (int r = std::min(in.pool_slots_max, 65534); r >= 64 && slots == 0; --r) {
      int cp = 1;
      while (cp < r) cp <<= 1;
      if (lds + (size_t)3 * cp * sizeof(uint32_t) + (size_t)r * 112 <= kLdsBytes) {
        slots = r;
        ring = cp;
      }
    }
    if (slots) {
      p.pool_ctl_off = (int)ctl;
      p.pool_ring_off = (int)lds;
      lds += (size_t)3 * ring * sizeof(uint32_t);
      p.pool_rec_off = (int)lds;
      lds += (size_t)slots * 112;
      p.pool_cap = ring;
      p.pool_slots = slots;
    }
  }
  p.lds = lds;
  return p;
}

}  // namespace

LdsPlan PlanLds(const BuildConsts& k, const LdsPlanIn& in) {
  // LDS mode: the whole scene + every lane's 2-dword stack fit in one CU's LDS (node pairs at the padded
  // LDS stride; only for node arrays whose pairs are all 64-B aligned)
  const size_t lds_mode_bytes = ((size_t)in.nodes_lds_f4 + (size_t)in.tris_f4) * kF4 +
                                (size_t)k.lds_block * 2 * sizeof(uint32_t) * (size_t)in.stack_entries;
  const bool ldsm = in.show_model && in.lds_ok && in.pairs_aligned && !in.force_global && lds_mode_bytes <= kLdsBytes;
  // pool mode (pool.hpp): LDS mode with stacks for the traversal waves only, then the ray records;
  // sample_kernel's layout when no 64 records fit
  if (ldsm && in.pool) {
    const LdsPlan p = Layout(k, in, true, true);
    if (p.pool_slots) return p;
  }
  return Layout(k, in, ldsm, false);
}

ChunkPlan PlanChunks(int W, int local_rows, int npx, int nframes, bool wf, size_t lbuf_total, int pipe) {
  ChunkPlan c{};
  // sample buffer: as many frames per chunk as the buffer cap allows
  const size_t per_frame = (size_t)npx * kF4;
  // frames per launch: what the sample buffer holds, and n_tiles * frames < 2^31 (the kernel's batch index),
  // less 2^20: the batch counter overshoots the end by up to (max(kClaim, kClaimSph) + 1) claims per wave;
  // wavefront mode (global-scene, timed launches): its sample items (64 per batch) < 2^31 per chunk
  c.n_tiles = (size_t)((W + 7) >> 3) * (size_t)((local_rows + 7) >> 3);
  c.max_frames = std::max<size_t>(
      1, ((size_t)0x7FFFFFFF - ((size_t)1 << 20)) / std::max<size_t>(1, c.n_tiles) / (wf ? 64 : 1));
  // the context's sample buffers share SRT_SAMPLE_BUFFER_MB: its own and, with pipeline slots, one per slot
  c.lbuf_cap = lbuf_total / (size_t)(pipe > 1 ? pipe + 1 : 1);
  c.chunk = (int)std::max<size_t>(
      1, std::min<size_t>(std::min<size_t>((size_t)nframes, c.max_frames), c.lbuf_cap / per_frame));
  c.need = per_frame * (size_t)c.chunk;
  c.nchunks = (nframes + c.chunk - 1) / c.chunk;
  return c;
}

}  // namespace srt
