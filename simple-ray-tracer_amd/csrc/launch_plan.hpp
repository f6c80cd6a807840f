// launch_plan.hpp -- pure host arithmetic of a sample launch: the LDS layout (LDS mode, global-scene mode
// or pool mode; stacks or rings, the COOP stages, the top-region copy, light / material records, the pool's
// rings and records) and the frames per chunk.  No device, no HIP header: pathtrace.hip's Launch reads the
// plan and does the device work; tests/cpp/test_launch_plan.cpp links launch_plan.cpp alone.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace srt {

// The constants of the device headers that host arithmetic needs.  They depend on macros an experiment build
// sets on the hipcc line only, so the host compiler must not define them a second time: pathtrace.hip fills
// this struct once from the headers it includes, and the plans and the scene image take every value from it.
struct BuildConsts {
  int lds_block;             // kLdsBlock: LDS mode's lanes per block
  int gw5_block;             // kGw5Block: the timed fused 5-wave instance's lanes per block
  uint32_t node_blk_f4;      // kNodeBlkF4: float4 per block of two node pairs in an LDS copy
  int ring_gw4, ring_gw5;    // global_ring(4), global_ring(5): ring entries per lane
  bool coop;                 // SRT_COOP
  uint32_t coop_wave_bytes;  // kCoopWaveBytes
  uint32_t coop_idx_bits;    // kCoopIdxBits
  int pool_trav_lanes;       // kPoolTravLanes
  uint32_t node_pad;         // kNodePad
  uint32_t tri_pad;          // kTriPad
  uint32_t treelet_cnt;      // kTreeletCnt
};

// LDS budget per CU (gfx950: 160 KiB; one 1024-thread block per CU in LDS mode)
constexpr size_t kLdsBytes = 160 * 1024;
// Lanes per block of a global-scene launch of `gw` waves per SIMD (timed fused instance or not)
constexpr int GlobalBlock(const BuildConsts& k, bool timed_fused, int gw) {
  return (timed_fused && gw == 5) ? k.gw5_block : 256;
}
// gfx950 hands a block its LDS in units of 1/128 of the CU's 160 KiB (1,280 B), so n blocks run together
// only when each asks at most floor(128 / n) units: 5 blocks fit at 32,000 B each, not at 32,001, while
// hipOccupancyMaxActiveBlocksPerMultiprocessor still answers 5 up to 32,768 (and 3, 6, 7 likewise past their
// limits; tools/probes/lds_fit.hip, profiles/r06_experiments/lds_fit.json).  The blocks per CU a launch's LDS
// size allows:
constexpr size_t kLdsGran = kLdsBytes / 128;
constexpr int LdsBlocksPerCu(size_t lds) { return lds == 0 ? 1 << 30 : (int)(128 / ((lds + kLdsGran - 1) / kLdsGran)); }
// The occupancy API's resident blocks per CU, capped by that allocation rule
inline int ResidentPerCu(int api_per_cu, size_t lds) { return std::max(1, std::min(api_per_cu, LdsBlocksPerCu(lds))); }
// The LDS one such block may take: its whole units of the CU's 160 KiB at gw waves per SIMD (4 SIMDs x 64
// lanes, gw * 256 / block blocks per CU)
constexpr size_t GlobalBlockLds(int block, int gw) { return (128 / ((size_t)gw * 256 / (size_t)block)) * kLdsGran; }
static_assert(GlobalBlockLds(256, 5) == 32000 && GlobalBlockLds(256, 4) == 40960 && GlobalBlockLds(640, 5) == 81920,
              "the LDS shares the probe measured");

// The pieces of a layout, shared by PlanLds and TopRegionBudget.
constexpr size_t kF4 = 16;  // bytes of a float4
constexpr size_t Align16(size_t b) { return (b + 15) & ~(size_t)15; }
// Packed stack / ring entries (2 dwords, else 3): indices below 2^24 and leaves below 256 triangles
constexpr bool PackedEntries(uint32_t n_tri_slots, uint32_t n_node_slots, uint32_t max_leaf, const BuildConsts& k) {
  return n_tri_slots < (1u << 24) && n_node_slots + k.node_pad < (1u << 24) && max_leaf < 256;
}
// A global-scene block's rings of stack entries
constexpr size_t RingBytes(const BuildConsts& k, int block, bool pack, int gw) {
  return (size_t)block * (pack ? 2 : 3) * sizeof(uint32_t) * (size_t)(gw == 5 ? k.ring_gw5 : k.ring_gw4);
}
// The LDS copy of a top region of `top_f4` float4 (padded pair blocks)
constexpr size_t TopRegionBytes(const BuildConsts& k, size_t top_f4) { return (top_f4 + 3) / 4 * k.node_blk_f4 * kF4; }
// LDS bytes of the light records a launch keeps in LDS (with the zero record), when they fit the kernel's cap
constexpr size_t LightLdsBytes(size_t light_records) {
  return 2 * kF4 * (light_records + 1) <= 8192 ? 2 * kF4 * (light_records + 1) : 0;
}

// What srt_upload_scene may spend on the fused instance's top region: the block's share less its rings and
// the light records set at upload -- at least the reference's six (src/main.cpp:584-589) -- and 64 B of
// alignment slack; the material records take what the region leaves.
// This is not the test PlanLds makes at launch ("two LDS budgets"): PlanLds places the region
// behind the rings *and the COOP stages*, beside the light records bound *at launch*.  With more lights by
// then (7 to 255), or in a COOP build, a region sized here can miss that test, and the launch drops it
// whole (launch.top_f4 = 0): the node layout is fixed at upload.  tests/cpp/test_launch_plan.cpp pins both.
constexpr size_t TopRegionBudget(const BuildConsts& k, int global_waves, bool pack, size_t lights_at_upload) {
  const int block = GlobalBlock(k, true, global_waves);
  const size_t share = GlobalBlockLds(block, global_waves);
  const size_t used = RingBytes(k, block, pack, global_waves) + LightLdsBytes(std::max<size_t>(lights_at_upload, 6)) + 64;
  return share > used ? share - used : 0;
}

struct LdsPlanIn {
  bool show_model, count;
  bool lds_ok, pairs_aligned, force_global, fused;  // of the uploaded scene (srt_context)
  int global_waves;
  bool pool;       // pool mode wanted (SRT_POOL, no sampled textures, max_depth in 0..255)
  int pool_slots_max;
  bool wavefront;  // wavefront mode wanted for timed global-scene launches
  int nodes_lds_f4, tris_f4, stack_entries, light_records;
  uint32_t n_mats;
  bool has_mats;   // material records uploaded
  int top_f4;      // the scene's top region (0: none)
};

// Everything Launch writes into KParams and the context's launch_* fields from the layout.  Offsets in
// float4 (_f4) or bytes (_off); a part the launch does without is 0.
struct LdsPlan {
  bool ldsm, pool, wf;  // LDS mode / pool mode / a wavefront launch
  int block, gw;        // lanes per block, waves per SIMD of a global-scene instance
  size_t lds;           // dynamic LDS bytes of the launch
  int stack_base_f4, coop_off, top_f4, top_lds_f4;
  int lights_lds, lights_base_f4, mats_lds, mat_records, mats_base_f4;
  int pool_ctl_off, pool_ring_off, pool_rec_off, pool_cap, pool_slots;
};
LdsPlan PlanLds(const BuildConsts& k, const LdsPlanIn& in);

// Frames per chunk of a launch of `nframes` frames of `npx` pixels (npx > 0) in 8x8 tiles.
struct ChunkPlan {
  size_t n_tiles, max_frames, lbuf_cap, need;  // need: sample buffer bytes of one chunk
  int chunk, nchunks;
};
ChunkPlan PlanChunks(int W, int local_rows, int npx, int nframes, bool wf, size_t lbuf_total, int pipe);

}  // namespace srt
