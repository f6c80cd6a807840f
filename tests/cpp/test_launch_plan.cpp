// The LDS layout and the chunking of a sample launch (csrc/launch_plan.cpp) as a stand-alone program, meant
// for AddressSanitizer + UBSan on the CPU (no device, no HIP):
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined tests/cpp/test_launch_plan.cpp
//       simple-ray-tracer_amd/csrc/launch_plan.cpp -o test_launch_plan && ./test_launch_plan
// Small numbers at the edges where the plan flips.
#include <cstdio>
#include <cstring>

#include "../../simple-ray-tracer_amd/csrc/launch_plan.hpp"

using namespace srt;

static int g_fail = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
      ++g_fail;                                                            \
    }                                                                      \
  } while (0)

// The product build's constants (kernels.hpp, traversal.hpp, pool.hpp at their defaults) but for node blocks
// of 4 float4 (an SRT_NODE_PAD=0 build: a region's bytes are then 16 per float4; TestTopRegion takes 5 too), a
// COOP build's (8-entry rings at either wave count) and an SRT_GW5_BLOCK=640 build's.
static constexpr BuildConsts kProduct = {1024, 256, 4, 16, 8, false, 24 * 128 + 256, 29, 64 * 14, 2, 3, 255};
static constexpr BuildConsts kCoop = {1024, 256, 4, 8, 8, true, 24 * 128 + 256, 29, 64 * 14, 2, 3, 255};
static constexpr BuildConsts kGw5Wide = {1024, 640, 4, 16, 8, false, 24 * 128 + 256, 29, 64 * 14, 2, 3, 255};

// A timed global-scene launch of the fused 5-wave instance: 256 lanes x 2 dwords x 8 entries = 16,384 B of rings.
static LdsPlanIn Global() {
  LdsPlanIn in{};
  in.show_model = true;
  in.lds_ok = in.pairs_aligned = in.fused = true;
  in.force_global = true;
  in.global_waves = 5;
  in.pool_slots_max = 4096;
  in.nodes_lds_f4 = 1000;
  in.tris_f4 = 3000;
  in.stack_entries = 10;
  in.light_records = 6;
  in.n_mats = 3;
  in.has_mats = true;
  return in;
}
// An LDS-mode launch: scene + 1024 lanes' stacks of `entries` 2-dword entries.
static LdsPlanIn Resident(int scene_f4, int entries) {
  LdsPlanIn in = Global();
  in.force_global = false;
  in.nodes_lds_f4 = scene_f4 / 4;
  in.tris_f4 = scene_f4 - scene_f4 / 4;
  in.stack_entries = entries;
  return in;
}
static bool Same(const LdsPlan& a, const LdsPlan& b) {
  return a.ldsm == b.ldsm && a.pool == b.pool && a.wf == b.wf && a.block == b.block && a.gw == b.gw && a.lds == b.lds &&
         a.stack_base_f4 == b.stack_base_f4 && a.coop_off == b.coop_off && a.top_f4 == b.top_f4 &&
         a.top_lds_f4 == b.top_lds_f4 && a.lights_lds == b.lights_lds && a.lights_base_f4 == b.lights_base_f4 &&
         a.mats_lds == b.mats_lds && a.mat_records == b.mat_records && a.mats_base_f4 == b.mats_base_f4 &&
         a.pool_ctl_off == b.pool_ctl_off && a.pool_ring_off == b.pool_ring_off && a.pool_rec_off == b.pool_rec_off &&
         a.pool_cap == b.pool_cap && a.pool_slots == b.pool_slots;
}

static void TestLdsModeBoundary() {
  // 8 stack entries: 1024 x 8 x 8 B = 64 KiB of stacks, so a 96-KiB scene (6,144 float4) makes exactly 160 KiB
  LdsPlan p = PlanLds(kProduct, Resident(6144, 8));
  CHECK(p.ldsm && !p.pool && !p.wf && p.block == 1024 && p.stack_base_f4 == 6144);
  CHECK(p.lds == kLdsBytes && !p.lights_lds && !p.mats_lds);  // nothing left for the records
  p = PlanLds(kProduct, Resident(6145, 8));
  CHECK(!p.ldsm && p.block == 256 && p.gw == 5 && p.stack_base_f4 == 0);
  // the other conditions of LDS mode
  LdsPlanIn in = Resident(1000, 8);
  CHECK(PlanLds(kProduct, in).ldsm);
  in.lds_ok = false;
  CHECK(!PlanLds(kProduct, in).ldsm);
  in = Resident(1000, 8);
  in.pairs_aligned = false;
  CHECK(!PlanLds(kProduct, in).ldsm);
  in = Resident(1000, 8);
  in.force_global = true;
  CHECK(!PlanLds(kProduct, in).ldsm);
  // records behind the stacks: lights at a 16-B aligned offset, then the materials
  p = PlanLds(kProduct, Resident(1000, 9));
  CHECK(p.lights_lds && p.lights_base_f4 == (1000 * 16 + 1024 * 8 * 9) / 16 && p.mats_lds && p.mat_records == 4);
  CHECK(p.mats_base_f4 == p.lights_base_f4 + 2 * 7 && p.lds == (size_t)(p.mats_base_f4 + 2 * 4) * 16);
  // the sphere scene: light records only
  in = Global();
  in.show_model = false;
  p = PlanLds(kProduct, in);
  CHECK(!p.ldsm && p.lights_lds && p.lights_base_f4 == 0 && !p.mats_lds && p.lds == 2 * 16 * 7 && p.top_f4 == 0);
}

static void TestGlobalShares() {
  static_assert(GlobalBlockLds(256, 5) == 32000 && GlobalBlockLds(256, 4) == 40960 && GlobalBlockLds(640, 5) == 81920, "");
  static_assert(LdsBlocksPerCu(32000) == 5 && LdsBlocksPerCu(32001) == 4 && LdsBlocksPerCu(0) == 1 << 30, "");
  static_assert(LdsBlocksPerCu(kLdsBytes) == 1 && LdsBlocksPerCu(kLdsBytes / 2) == 2 && LdsBlocksPerCu(kLdsBytes / 2 + 1) == 1, "");
  CHECK(ResidentPerCu(8, 32000) == 5 && ResidentPerCu(8, 32001) == 4 && ResidentPerCu(3, 32000) == 3 && ResidentPerCu(0, 0) == 1);
  CHECK(GlobalBlock(kProduct, true, 5) == 256 && GlobalBlock(kGw5Wide, true, 5) == 640 && GlobalBlock(kGw5Wide, true, 4) == 256 &&
        GlobalBlock(kGw5Wide, false, 5) == 256);
  // the instance: 5 waves only for a timed fused launch; a counting one takes 4 waves and 16-entry rings
  LdsPlanIn in = Global();
  LdsPlan p = PlanLds(kProduct, in);
  CHECK(p.gw == 5 && p.block == 256 && p.lights_base_f4 == 256 * 8 * 8 / 16);
  in.count = true;
  p = PlanLds(kProduct, in);
  CHECK(p.gw == 4 && p.block == 256 && p.lights_base_f4 == 256 * 8 * 16 / 16);
  in = Global();
  in.lds_ok = false;  // 3-dword entries
  CHECK(PlanLds(kProduct, in).lights_base_f4 == 256 * 12 * 8 / 16);
  CHECK(PlanLds(kGw5Wide, Global()).block == 640 && PlanLds(kGw5Wide, Global()).lights_base_f4 == 640 * 8 * 8 / 16);
}

static void TestRecords() {
  // light records: 2 x 16 x (n + 1) <= 8192
  LdsPlanIn in = Global();
  in.light_records = 255;
  LdsPlan p = PlanLds(kProduct, in);
  CHECK(p.lights_lds == 1 && LightLdsBytes(255) == 8192 && p.mats_base_f4 == p.lights_base_f4 + 512);
  in.light_records = 256;
  p = PlanLds(kProduct, in);
  CHECK(p.lights_lds == 0 && LightLdsBytes(256) == 0 && p.lights_base_f4 == 0 && p.mats_lds == 1);
  // material records: 2 x 16 x (n + 1) <= 16384
  // (in 640-lane blocks, whose share of 81,920 B holds them beside 40,960 B of rings)
  in = Global();
  in.n_mats = 511;
  p = PlanLds(kGw5Wide, in);
  CHECK(p.mats_lds == 1 && p.mat_records == 512 && p.lds == 40960 + 224 + 16384);
  in.n_mats = 512;
  p = PlanLds(kGw5Wide, in);
  CHECK(p.mats_lds == 0 && p.mat_records == 513 && p.mats_base_f4 == 0 && p.lds == 40960 + 224);
  in.n_mats = 3;
  in.has_mats = false;
  CHECK(PlanLds(kGw5Wide, in).mats_lds == 0);
  // both beyond the share (32,000 B at 5 waves): the region stays, the materials go to HBM
  in = Global();
  in.n_mats = 400;                                   // 12,832 B
  in.top_f4 = 4 * ((32000 - 16384 - 224 - 6000) / 64);  // 9,344 B of region: 6,048 B left
  p = PlanLds(kProduct, in);
  CHECK(p.top_f4 == in.top_f4 && p.top_lds_f4 == 16384 / 16 && p.lights_lds == 1 && p.mats_lds == 0);
  CHECK(p.lds == 16384 + 9344 + 224 && TopRegionBytes(kProduct, (size_t)in.top_f4) == 9344);
  in.top_f4 = 0;
  CHECK(PlanLds(kProduct, in).mats_lds == 1);
}

static void TestTopRegion() {
  // kept when rings + region + lights <= share (32,000): 16,384 + tb + 224, so tb <= 15,392 = 240.5 blocks of 64 B
  LdsPlanIn in = Global();
  in.n_mats = 0;
  in.top_f4 = 4 * 240;
  LdsPlan p = PlanLds(kProduct, in);
  CHECK(p.top_f4 == 4 * 240 && p.top_lds_f4 == 1024 && p.lights_base_f4 == 1024 + 4 * 240);
  in.top_f4 = 4 * 240 + 2;  // one block of four pairs more (a region ends on a pair: 2 float4 into the block)
  p = PlanLds(kProduct, in);
  CHECK(p.top_f4 == 0 && p.top_lds_f4 == 0 && p.lights_base_f4 == 1024);
  // a node block of 5 float4 (SRT_NODE_PAD builds)
  BuildConsts padded = kProduct;
  padded.node_blk_f4 = 5;
  in.top_f4 = 4 * 192;  // 192 x 80 = 15,360
  CHECK(PlanLds(padded, in).top_f4 == in.top_f4);
  in.top_f4 = 4 * 193;
  CHECK(PlanLds(padded, in).top_f4 == 0);
  // never for a counting, non-fused or wavefront launch
  in = Global();
  in.top_f4 = 64;
  CHECK(PlanLds(kProduct, in).top_f4 == 64);
  in.count = true;
  CHECK(PlanLds(kProduct, in).top_f4 == 0);
  in = Global();
  in.top_f4 = 64;
  in.fused = false;
  CHECK(PlanLds(kProduct, in).top_f4 == 0 && PlanLds(kProduct, in).gw == 4);
  in = Global();
  in.top_f4 = 64;
  in.wavefront = true;
  p = PlanLds(kProduct, in);
  CHECK(p.top_f4 == 0 && p.wf);
  in.count = true;  // (a counting launch is never a wavefront one)
  CHECK(!PlanLds(kProduct, in).wf);
  CHECK(!PlanLds(kProduct, Resident(1000, 8)).wf);
}

static void TestPool() {
  // scene + 896 traversal lanes' stacks + records, then 64 B of control words, rings and 112-B records
  LdsPlanIn in = Resident(1000, 8);
  in.pool = true;
  LdsPlan p = PlanLds(kProduct, in);
  const LdsPlan plain = PlanLds(kProduct, Resident(1000, 8));
  CHECK(p.pool && p.ldsm && p.stack_base_f4 == 1000 && p.pool_ctl_off == 1000 * 16 + 896 * 64 + 224 + 128);
  CHECK(p.pool_ring_off == p.pool_ctl_off + 64 && p.pool_rec_off == p.pool_ring_off + 3 * 4 * p.pool_cap);
  CHECK(p.lds == (size_t)p.pool_rec_off + (size_t)p.pool_slots * 112 && p.lds <= kLdsBytes);
  // the largest count that fits: 163,840 - 73,696 - 64 = 90,080 B; 3 x 4 x 1024 + 112 r <= 90,080 -> r = 694
  CHECK(p.pool_slots == 694 && p.pool_cap == 1024);
  CHECK((size_t)p.pool_rec_off + 695 * 112 > kLdsBytes);
  in.pool_slots_max = 500;
  p = PlanLds(kProduct, in);
  CHECK(p.pool_slots == 500 && p.pool_cap == 512);
  in.pool_slots_max = 1 << 20;  // (record ids are 16 bits)
  CHECK(PlanLds(kProduct, in).pool_slots == 694);
  // room for 64 records exactly: 64 + 3 x 4 x 64 + 64 x 112 = 8,000 B behind the rest; one float4 more, none
  // (one stack entry: with more, the 128 lanes' stacks pool mode saves exceed those 8,000 B, and a scene that
  // leaves them to pool mode is too large for LDS mode)
  in = Resident(1000, 1);
  in.pool = true;
  in.light_records = 300;  // (no records in LDS: the layout is scene + stacks)
  in.has_mats = false;
  in.tris_f4 += (int)((kLdsBytes - 1000 * 16 - 896 * 8 - 8000) / 16);
  p = PlanLds(kProduct, in);
  CHECK(p.pool && p.pool_slots == 64 && p.pool_cap == 64 && p.lds == kLdsBytes);
  in.tris_f4 += 1;
  p = PlanLds(kProduct, in);
  LdsPlanIn same = in;
  same.pool = false;
  CHECK(!p.pool && p.pool_slots == 0 && p.pool_ctl_off == 0 && Same(p, PlanLds(kProduct, same)));
  CHECK(!Same(PlanLds(kProduct, Resident(1000, 8)), PlanLds(kProduct, Resident(1000, 9))));  // (Same can tell plans apart)
  // the fallback keeps LDS mode only while every lane's stack fits; pool mode never runs outside it
  CHECK(!plain.pool && plain.pool_slots == 0);
  in = Global();
  in.pool = true;
  CHECK(!PlanLds(kProduct, in).pool);
}

static void TestCoop() {
  LdsPlanIn in = Global();
  in.light_records = 0;
  LdsPlan p = PlanLds(kCoop, in);
  // rings of SRT_RING_GW5 = 8 entries at either wave count, then 4 stages of 3,328 B at a 16-B aligned offset
  CHECK(p.coop_off == 256 * 8 * 8 && p.coop_off % 16 == 0 && p.lights_base_f4 == (p.coop_off + 4 * 3328) / 16);
  in.global_waves = 4;
  CHECK(PlanLds(kCoop, in).coop_off == 256 * 8 * 8 && PlanLds(kProduct, in).coop_off == 0);
  in.lds_ok = false;
  // (a block is a multiple of 64 lanes, so rings of whole dwords end 16-B aligned at every entry count)
  BuildConsts odd = kCoop;
  odd.gw5_block = 320;
  odd.ring_gw5 = 7;
  in.global_waves = 5;
  p = PlanLds(odd, in);
  CHECK(p.block == 320 && p.coop_off == 320 * 12 * 7 && p.coop_off % 16 == 0);
  // counting launches have no stages
  in.count = true;
  CHECK(PlanLds(kCoop, in).coop_off == 0);
}

// ADVICE.md, "two LDS budgets": the upload sizes the region beside max(lights set, 6) light records and no
// COOP stages; the launch tests it beside the records bound by then and the stages.  What happens today:
static void TestTwoBudgets() {
  const size_t budget = TopRegionBudget(kProduct, 5, true, 0);
  CHECK(budget == 32000 - 16384 - 224 - 64 && budget == TopRegionBudget(kProduct, 5, true, 6));
  CHECK(TopRegionBudget(kProduct, 5, true, 7) == budget - 32 && TopRegionBudget(kProduct, 5, true, 256) == budget + 224);
  CHECK(TopRegionBudget(kProduct, 4, false, 6) == 0);  // 3-dword 16-entry rings take 49,152 B: no region
  CHECK(TopRegionBudget(kProduct, 4, true, 6) == 40960 - 32768 - 224 - 64);
  // the largest region the upload accepts at six lights: 239 blocks (15,296 B <= 15,328)
  LdsPlanIn in = Global();
  in.n_mats = 0;
  in.top_f4 = 4 * 239;
  CHECK(TopRegionBytes(kProduct, (size_t)in.top_f4) <= budget && TopRegionBytes(kProduct, (size_t)in.top_f4 + 4) > budget);
  CHECK(PlanLds(kProduct, in).top_f4 == in.top_f4);  // six lights at launch: kept
  in.light_records = 7;  // 64 B of slack = two more records: kept with 7 to 9 ...
  CHECK(PlanLds(kProduct, in).top_f4 == in.top_f4);
  in.light_records = 9;
  CHECK(PlanLds(kProduct, in).top_f4 == in.top_f4);
  in.light_records = 10;  // ... and dropped whole from 10 on (16,384 + 15,296 + 352 > 32,000)
  LdsPlan p = PlanLds(kProduct, in);
  CHECK(p.top_f4 == 0 && p.top_lds_f4 == 0 && p.lights_lds == 1);
  in.light_records = 255;
  p = PlanLds(kProduct, in);
  CHECK(p.top_f4 == 0 && p.lights_lds == 1);
  in.light_records = 256;  // past the 8-KB cap the records stay in HBM and the region is back
  CHECK(PlanLds(kProduct, in).top_f4 == in.top_f4);
  // a COOP build: the stages (4 x 3,328 B) are no part of the budget, so the same region is dropped at six lights
  in.light_records = 6;
  CHECK(TopRegionBudget(kCoop, 5, true, 6) == budget && PlanLds(kCoop, in).top_f4 == 0);
}

static void TestChunks() {
  // 1920 x 1080: 240 x 135 = 32,400 tiles
  ChunkPlan c = PlanChunks(1920, 1080, 1920 * 1080, 1 << 20, false, (size_t)64 << 30, 2);
  CHECK(c.n_tiles == 32400 && c.max_frames == (0x7FFFFFFFull - (1 << 20)) / 32400);
  CHECK(c.n_tiles * c.max_frames < (1ull << 31) - (1 << 20) + 1 && c.n_tiles * (c.max_frames + 1) > (1ull << 31) - (1 << 20));
  CHECK(c.lbuf_cap == ((size_t)64 << 30) / 3 && c.chunk == (int)(c.lbuf_cap / (1920 * 1080 * 16)));
  CHECK(c.need == (size_t)c.chunk * 1920 * 1080 * 16 && c.nchunks == ((1 << 20) + c.chunk - 1) / c.chunk);
  // the tile bound binds: a large buffer, and wavefront mode's 64 items per batch
  c = PlanChunks(1920, 1080, 1920 * 1080, 1 << 20, false, (size_t)1 << 50, 1);
  CHECK(c.lbuf_cap == (size_t)1 << 50 && c.chunk == (int)c.max_frames && (size_t)c.chunk * c.n_tiles < (1ull << 31) - (1 << 20));
  const ChunkPlan w = PlanChunks(1920, 1080, 1920 * 1080, 1 << 20, true, (size_t)1 << 50, 1);
  CHECK(w.max_frames == c.max_frames / 64 && 64 * w.n_tiles * (size_t)w.chunk < (1ull << 31) - (1 << 20));
  // the cap is shared by pipe + 1 buffers (none extra without slots)
  CHECK(PlanChunks(64, 64, 4096, 8, false, 3 << 20, 2).lbuf_cap == 1 << 20);
  CHECK(PlanChunks(64, 64, 4096, 8, false, 3 << 20, 1).lbuf_cap == 3 << 20);
  CHECK(PlanChunks(64, 64, 4096, 8, false, 3 << 20, 0).lbuf_cap == 3 << 20);
  c = PlanChunks(64, 64, 4096, 100, false, 3 << 20, 2);  // 64 KiB a frame: 16 per chunk
  CHECK(c.chunk == 16 && c.nchunks == 7 && c.need == 1 << 20 && c.n_tiles == 64);
  c = PlanChunks(64, 64, 4096, 5, false, 3 << 20, 2);  // fewer frames than a chunk holds
  CHECK(c.chunk == 5 && c.nchunks == 1 && c.need == 5 * 65536);
  // one frame exceeds the cap: still one frame per chunk
  c = PlanChunks(64, 64, 4096, 3, false, 1000, 2);
  CHECK(c.chunk == 1 && c.nchunks == 3 && c.need == 65536);
  // tiles round up, rows of a rank's share
  CHECK(PlanChunks(65, 9, 65 * 9, 1, false, 1 << 30, 2).n_tiles == 9 * 2);
  // the largest image FillParams accepts: 8192 x 4096 tiles, (2^31 - 2^20 - 1) / 2^25 = 63 frames; none in wavefront mode
  c = PlanChunks(65535, 32767, 65535 * 32767, 100, false, (size_t)1 << 50, 1);
  CHECK(c.n_tiles == (size_t)1 << 25 && c.max_frames == 63 && c.chunk == 63 && c.nchunks == 2);
  c = PlanChunks(65535, 32767, 65535 * 32767, 100, true, (size_t)1 << 50, 1);
  CHECK(c.max_frames == 1 && c.chunk == 1 && c.nchunks == 100);  // (floor(63 / 64) = 0: still one frame)
}

int main() {
  TestLdsModeBoundary();
  TestGlobalShares();
  TestRecords();
  TestTopRegion();
  TestPool();
  TestCoop();
  TestTwoBudgets();
  TestChunks();
  if (g_fail) {
    std::fprintf(stderr, "%d check(s) failed\n", g_fail);
    return 1;
  }
  std::printf("launch plan checks OK\n");
  return 0;
}
