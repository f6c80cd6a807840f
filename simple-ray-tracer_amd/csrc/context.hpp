// context.hpp -- the device context behind the C ABI, declared once: context.cpp holds its host-only
// part (create / destroy, uniforms, lights, noise, images, checkpoints, statistics, kernel time) and
// pathtrace.hip the part that launches kernels.  Compiles under the host compiler: the HIP runtime API
// and HIP's vector types only, no device header.
#pragma once

#include <hip/hip_runtime_api.h>
#include <hip/hip_vector_types.h>

#include <cstddef>
#include <cstdint>
#include <string>
#include <utility>
#include <vector>

#include "srt_internal.hpp"
#include "tile_cull.hpp"

#define HIP_OK(expr)                                                                          \
  do {                                                                                        \
    hipError_t e_ = (expr);                                                                   \
    if (e_ != hipSuccess) {                                                                   \
      srt::SetError(std::string(#expr) + ": " + hipGetErrorString(e_));                     \
      return SRT_ERR_HIP;                                                                     \
    }                                                                                         \
  } while (0)

struct srt_context {
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  // uniforms
  int W = 0, H = 0, accum_frames = 0, reset = 0, show_model = 0, light_count = 0, max_depth = 5;
  uint32_t bvh_count = 0;
  float cam_origin[3] = {0, 0, 0}, cam_dir[3] = {0, 0, -1}, cam_up[3] = {0, 1, 0}, cam_right[3] = {1, 0, 0};
  // tiling
  int rank = 0, nranks = 1, band_rows = 16;
  // scene
  float4* d_nodes = nullptr;
  float4* d_tris = nullptr;
  float4* d_mats = nullptr;
  srt_bvh_record* d_bvhs = nullptr;
  uint32_t bvh_capacity = 0;
  uint32_t bvh_uploaded = 0;   // records on the device (valid while !bvhs_dirty)
  bool bvhs_dirty = true;
  std::vector<srt_bvh_record> h_bvhs;
  std::vector<std::pair<uint32_t, uint32_t>> bvh_tris;  // triangle range [lo, hi) of each record's tree
  uint32_t n_nodes = 0, n_tris = 0, n_mats = 0;
  uint32_t ref_or = 0;  // KParams::ref_or of the uploaded node layout
  // textures (srt_upload_textures) and, when materials sample them, the
  // per-triangle vertex uvs (2 float4: uv0 uv1 | uv2 0 0)
  void* d_tex = nullptr;         // texels: RGBA8 (SRT_TEX8) or RGBA32F
  uint4* d_tex_info = nullptr;  // first texel, width, height, 0
  uint32_t n_tex = 0;
  float4* d_tri_uv = nullptr;
  bool sample_textures = false;
  int stack_entries = 1;
  bool scene_ok = false;
  bool lds_ok = false;        // scene indices fit the packed LDS stack entry
  bool pairs_aligned = false; // every internal node's child pair starts at an odd slot (LDS mode's node_pair)
  bool force_global = false;  // SRT_FORCE_GLOBAL_SCENE=1 disables LDS mode
  bool fused = false;         // global-scene mode's fused sub-steps (set at upload: trees the Infinity Cache holds)
  int top_f4 = 0, top_depth = 0;  // the node array's top-level region (LayoutNodes) the fused instance copies to LDS
  int launch_top_f4 = 0;           // the region the last global-scene launch copied (0: none)
  bool launch_overlap = false;     // the last render's sample launches ran piped and overlapped (launch.overlap)
  int launch_per_cu = 0, launch_block = 0;  // resident blocks per CU and lanes per block of the last sample launch
  int launch_mats_lds = 0;                  // the last launch read the material records from LDS
  int global_waves = 4;       // the fused instance's waves per SIMD (set at upload: 5 for small trees)
  // lights
  std::vector<srt_light> h_lights;
  float4* d_lights = nullptr;
  uint32_t light_capacity = 0;
  bool lights_dirty = true;
  // noise
  float2* d_noise_xy = nullptr;
  float* d_noise_u = nullptr;
  size_t noise_texels = 0;
  // images
  float4* d_accum = nullptr;
  uint32_t* d_out = nullptr;
  bool images_external = false;
  int img_w = 0, img_rows = 0;
  // sample buffer (nframes x local pixels float4)
  float4* d_lbuf = nullptr;
  uint32_t* d_gstack = nullptr;  // global-scene mode traversal stacks
  size_t gstack_bytes = 0;
  // tile schedule: per-tile costs recorded by the last launch and the next
  // launch's order (order_tiles_kernel); costs_for = the tile count they describe
  uint32_t* d_tile_cost = nullptr;
  uint32_t* d_tile_order = nullptr;
  int tile_cap = 0, tile_costs_for = -1;
  bool tile_schedule = true;  // SRT_TILE_ORDER=0: natural tile order
  // Tile culling (tile_cull.hpp): the timed launches of a mesh scene trace only the tiles that are not
  // provably sky.  The classification is recomputed when what it reads changes (cull_key: camera, extent,
  // frame, tiling, BVH records, noise, launch kind), never per chunk.  Its device copies go through a small
  // ring of buffers: a new map is written to pinned staging and copied on cull_stream into the next entry,
  // the launch's streams wait for that copy, and an entry is reused only after the last launch that read it
  // (its `used` event), which the host waits for.  No launch is drained, but that wait and the copy cost a
  // host that runs ahead of the GPU about 0.25 ms per new map, so a launch that culls fewer than
  // cull_min_samples samples keeps the map already on the device or runs all-live (pathtrace.hip EnsureTileCull).
  bool tile_cull = true;              // SRT_TILE_CULL=0: every tile stays live
  long long cull_min_samples = 1ll << 24;  // SRT_TILE_CULL_MIN_SAMPLES: culled samples a launch needs for a new map
  bool roots_ok = false;              // h_roots holds every uploaded record's root box
  std::vector<srt::RootBox> h_roots;  // root box of each uploaded record's tree
  std::vector<int> h_row_map;         // host copy of d_row_map
  float nz_min[2] = {0, 0}, nz_max[2] = {0, 0};  // extremes of noise_xy (srt_set_noise)
  bool noise_finite = false;
  unsigned long long cull_gen = 0;    // bumped by whatever the key cannot hold: BVH records, noise
  std::vector<unsigned char> cull_key;
  int cull_live = 0;                  // of the classification for cull_key: its live tiles, and the in-extent
  long long cull_pixels = 0;          // pixels of its sky tiles
  struct CullBuf {
    uint32_t* d_live = nullptr;       // the live tiles' indices, ascending
    uint8_t* d_sky = nullptr;         // per tile: 1 = sky
    uint32_t* h_live = nullptr;       // pinned staging of both
    uint8_t* h_sky = nullptr;
    int cap = 0;
    hipEvent_t ready = nullptr, used = nullptr;  // the copy has landed / the last launch reading it has ended
    bool ready_rec = false, used_rec = false;
  };
  static constexpr int kCullRing = 4;
  CullBuf cull_ring[kCullRing];
  int cull_cur = -1;                  // the entry holding h_tile_sky (-1: none yet)
  std::vector<uint8_t> h_tile_sky;    // the map in cull_ring[cull_cur]
  hipStream_t cull_stream = nullptr;
  unsigned long long cull_uploads = 0;  // maps sent to the device since create (cull.uploads)
  int launch_live_tiles = 0;          // of the last render's launches (launch.live_tiles)
  long long launch_culled = 0;        // samples the last render did not trace (launch.culled_samples)
  int* d_row_map = nullptr;           // nranks > 1: global row of each local row (KParams::row_map)
  long long row_map_key = -1;         // the (rank, nranks, band_rows, rows) it was built for
  unsigned long long* d_batch_ctr = nullptr;  // one batch counter per chunk launch
  int batch_ctr_cap = 0;
  size_t lbuf_bytes = 0;
  // SRT_SAMPLE_BUFFER_MB: every sample buffer of the context together (its own, used by counting and
  // unpipelined launches, and one per pipeline slot), split equally: 21 GiB each with the 2 default slots
  size_t lbuf_total = (size_t)64 << 30;
  int tail_claims = 16;  // SRT_TAIL_CLAIMS: claims per wave before the end from which claims take one batch
  int tail_claims_gw5 = 8;  // the untextured fused 5-wave instance's (torus knot +1.4% against 16 with two slots;
                            // the textured Airplane material loses 0.6% and keeps 16;
                            // profiles/r05_experiments/tail_window_overlap.txt); SRT_TAIL_CLAIMS sets it too
  int tail_claims_sph = 1;  // the sphere launch's (C2, 8 per claim: tail 16 6.20 ms, 1 3.17 ms; its batches
                            // are cheap, the counter's atomic rate bounds it); SRT_TAIL_CLAIMS sets both
  int trav_frac16 = 9;                 // SRT_TRAV_FRAC16 (measured best on Rubik 1080p with the 16-sub-step pattern)
  int bounce_cap = 1 << 20;            // SRT_BOUNCE_CAP: bounces after which a path is cut (counted)
  int trav_frac16_global = 9;          // SRT_TRAV_FRAC16_GLOBAL: the same threshold for global-scene mode
  bool trav_frac16_global_env = false; // (set: every global instance uses it; else the fused 4-wave one takes 7, the timed IL one 8)
  bool pool_launched = false;          // the last render ran pool_kernel (srt_finish checks its watchdog)
  int pool = 0;                        // SRT_POOL=1: LDS mode runs pool_kernel (workgroup ray pools)
  int pool_batch = 64;                 // SRT_POOL_BATCH: queued hits a shading wave waits for
  int pool_tlow = 32;                  // SRT_POOL_TLOW: trace + spare records under which shading waves take fewer
  int pool_slots_max = 4096;           // SRT_POOL_SLOTS: at most this many records
  int pool_deadline_ms = 30000;        // SRT_POOL_DEADLINE_MS: pool_kernel's watchdog
  int num_cus = 256;
  int sphere_blocks = 5;               // SRT_SPHERE_BLOCKS: sphere_kernel blocks per CU (at most)
  // wavefront mode (wavefront.hpp): global-scene launches through wf_logic / wf_shade / wf_trace
  int wavefront = -1;                  // SRT_WAVEFRONT=1/0 forces it on / off; -1: by scene (wf_scene)
  bool wf_scene = false;               // chosen at upload
  uint32_t wf_slots = 1u << 21;        // SRT_WF_SLOTS: path slots in HBM
  int wf_waves = 6;                    // SRT_WF_WAVES: waves per SIMD of wf_trace_kernel (4, 5, 6 or 8)
  float4* d_wf_rec = nullptr;
  uint2* d_wf_res = nullptr;
  uint32_t *d_wf_state = nullptr, *d_wf_rayq = nullptr, *d_wf_hitq = nullptr, *d_wf_ctl = nullptr,
           *d_wf_items = nullptr;
  uint32_t wf_cap = 0;
  uint32_t* h_wf_poll = nullptr;       // pinned: (live, items) of two polled iterations
  hipEvent_t wf_poll_ev[2] = {nullptr, nullptr};
  bool wf_launched = false;            // the last render went through wavefront mode
  // treelet scheduling of wavefront mode's trace stage (wavefront.hpp wf_top_kernel / wf_bottom_kernel)
  int treelets = -1;                   // SRT_TREELETS=1/0 forces it on / off; -1: by scene (tl_scene)
  bool tl_scene = false;               // chosen at upload
  int treelet_depth = 0;               // SRT_TREELET_DEPTH: depth of the treelet roots (0: by scene size)
  uint32_t n_treelets = 0;             // of the uploaded scene (0: no flagged copy)
  float4* d_nodes_t = nullptr;         // the node array with treelet roots flagged
  uint32_t* d_troot = nullptr;         // per treelet: its root's child index
  float4* d_tl_ray = nullptr;
  uint32_t *d_tl_stk = nullptr, *d_tl_slist = nullptr, *d_tl_skey = nullptr, *d_tl_blist = nullptr,
           *d_tl_rlist = nullptr, *d_tl_count = nullptr, *d_tl_fill = nullptr;
  uint32_t tl_cap = 0, tl_count_cap = 0;
  // stats
  unsigned long long* d_stats = nullptr;
  unsigned long long* d_nan = nullptr;  // NaN path samples since the last srt_reset_stats
  srt_stats stats{};
  uint64_t shadow_rays = 0;  // of stats.rays (srt_ray_kinds)
  // per-chunk HIP events around the sample kernel of the last render call
  std::vector<hipEvent_t> ev;
  struct Occupancy {
    const void* fn;
    size_t lds;
    int per_cu;
  };
  std::vector<Occupancy> occupancy;  // resident blocks per CU of each sample_kernel instance
  // (SRT_WAVE_TRACE builds use these; declared in every build, so that the files the host compiler
  // builds without that flag see the same layout)
  unsigned long long* d_trace = nullptr;
  size_t trace_bytes = 0;
  int trace_waves = 0;
  int ev_used = 0;
  // Pipelined sample launches (SRT_PIPELINE slots, default 3; 1: every launch on `stream`).  A timed
  // sample_kernel / sphere_kernel launch goes on the next slot's own stream with the slot's sample
  // buffer, batch counter, tile order and stacks; its accumulate_kernel stays on `stream` behind it.  A
  // slot's next launch waits only for that slot's last accumulation, so launch k+1 fills the CUs that
  // launch k's last waves leave idle (the drain) and the accumulations run beside them, instead of
  // sample and accumulate alternating on one stream.  The tile order of a slot's launch comes from the
  // costs of that slot's previous launch (the order decides which wave traces which sample, never a
  // value).  Counting, pool and wavefront launches run on `stream` with the context's own buffers.
  struct Slot {
    hipStream_t stream = nullptr;
    hipEvent_t sampled = nullptr, accumulated = nullptr;
    bool pending = false;  // `accumulated` recorded since the slot's buffers were last known idle
    float4* lbuf = nullptr;
    size_t lbuf_bytes = 0;
    unsigned long long* batch_ctr = nullptr;
    int batch_ctr_cap = 0;
    uint32_t* tile_cost = nullptr;
    uint32_t* tile_order = nullptr;
    int tile_cap = 0, tile_costs_for = -1;
    uint32_t* gstack = nullptr;
    size_t gstack_bytes = 0;
  };
  std::vector<Slot> slots;
  // SRT_PIPELINE: launch slots, each its own stream and buffers.  Two, since launches overlap: a third slot's
  // stream shares one of the process's 4 hardware queues (GPU_MAX_HW_QUEUES) with another, which serialises
  // them (C2 52 -> 57 G rays/s, torus knot +2.8%, metric +0.2% with 2)
  int pipe = 2;
  // SRT_PIPELINE_OVERLAP: whether a sample launch may start before the previous one ends (2, the default:
  // always; 1: on a rank's share of a multi-GPU split (nranks > 1) only; 0: never).  An overlapped launch's
  // dispatch-to-end time (rocprofv3) and span include its wait for the CUs other launches hold, so kernel
  // time is the union of the launches' spans (srt_kernel_time; tools/trace_intervals.py takes the same
  // union over rocprofv3's kernel trace).
  int pipe_overlap = 2;
  hipEvent_t last_sampled = nullptr;  // the last sample launch's end (a slot's `sampled`, or plain_done)
  hipEvent_t plain_done = nullptr;    // recorded on `stream` after a launch outside the slots
  unsigned long long pipe_seq = 0;
  hipStream_t lstream = nullptr;   // the stream the current launch's sample kernel goes on
  // Kernel time of sample_kernel / sphere_kernel launches: each writes its span (first wave's start,
  // last wave's end; s_memrealtime) into a record of this ring (HIP events around a pipelined launch
  // would also time its wait for the CUs its predecessor still holds).
  unsigned long long* d_span = nullptr;
  static constexpr int kSpanCap = 4096;
  unsigned long long span_seq = 0, span_read = 0;  // records written / summed by srt_kernel_time
  unsigned long long span_done = 0;                 // the latest end srt_kernel_time has counted (a tick)
  std::vector<long long> chunk_span;               // per chunk of the last render: its record (or -1)
  hipEvent_t lidle = nullptr;      // synchronized before the current launch frees a launch buffer
  hipEvent_t lidle2 = nullptr;     // (and this: the previous launch, for the buffers launches in series share)
};

namespace srt {

// context.cpp: helpers of both halves
const char* LastError();
void FreeDev(void* p);
int HipFail(const char* what);
// Waits until no pipelined sample launch is in flight: before anything rewrites or frees device data
// those launches read (scene, lights, BVH records, noise, row map).
int Quiesce(srt_context* c);
// Before the launch being set up frees one of its buffers: the launches that may still read it are done.
int WaitLaunchIdle(srt_context* c);
int LocalRows(const srt_context* c, int H);
// The device copies of the BVH records / light records, brought up to date before a launch reads them
int EnsureBvhs(srt_context* c);
int EnsureLights(srt_context* c);

}  // namespace srt
