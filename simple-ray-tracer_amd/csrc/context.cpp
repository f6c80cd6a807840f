// context.cpp -- the host-only part of the device context behind the C ABI (context.hpp): create and
// destroy, uniforms, tiling, light / noise uploads, image buffers and their I/O, checkpoints, statistics
// and kernel time.  Nothing here launches a kernel or reads a device header; pathtrace.hip holds the rest.
// Device layout of what this file uploads:
//   lights : 32 B, one zero record appended (lights[lightCount] reads zero);
//   noise  : noiseTex as .xy float2 (8 B), noiseUniformTex as .x float (4 B):
//            the only channels the kernel reads.
#include "context.hpp"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <mutex>

#include <zlib.h>

#include "scene_layout.hpp"

namespace srt {

static std::mutex g_err_mu;
static std::string g_err;
void SetError(const std::string& msg) {
  std::lock_guard<std::mutex> lk(g_err_mu);
  g_err = msg;
}
const char* LastError() {
  std::lock_guard<std::mutex> lk(g_err_mu);
  return g_err.c_str();
}

void FreeDev(void* p) {
  if (p) (void)hipFree(p);
}

int HipFail(const char* what) {
  const hipError_t e = hipGetLastError();
  srt::SetError(std::string(what) + ": " + hipGetErrorString(e));
  return SRT_ERR_HIP;
}

// Waits until no pipelined sample launch is in flight: before anything rewrites or frees device data
// those launches read (scene, lights, BVH records, noise, row map).
int Quiesce(srt_context* c) {
  for (auto& s : c->slots)
    if (s.stream) HIP_OK(hipStreamSynchronize(s.stream));
  return SRT_OK;
}

// Before the launch being set up frees one of its buffers: the launches that may still read it are done.
int WaitLaunchIdle(srt_context* c) {
  if (c->lidle) HIP_OK(hipEventSynchronize(c->lidle));
  if (c->lidle2) HIP_OK(hipEventSynchronize(c->lidle2));
  return SRT_OK;
}

int LocalRows(const srt_context* c, int H) {
  int rows = 0;
  const int nb = (H + c->band_rows - 1) / c->band_rows;
  for (int b = c->rank; b < nb; b += c->nranks) rows += std::min(c->band_rows, H - b * c->band_rows);
  return rows;
}

int EnsureBvhs(srt_context* c) {
  const uint32_t need = std::max<uint32_t>(c->bvh_count, 1);
  if (!c->bvhs_dirty && c->bvh_uploaded >= need) return SRT_OK;
  std::vector<srt_bvh_record> recs(need);
  std::memset(recs.data(), 0, sizeof(srt_bvh_record) * need);   // bvhs[i >= n] read as zeros
  for (uint32_t i = 0; i < need && i < c->h_bvhs.size(); ++i) {
    recs[i] = c->h_bvhs[i];
    // pad0/pad1 carry the triangle range of the record's tree, empty for a
    // record whose frame zeroes every direction (it never hits: the ghost
    // of src/main.cpp:683); texture sampling finds the hit's BVH by it
    const float* f = recs[i].frame;
    bool can_hit = false;
    for (int k : {0, 1, 2, 4, 5, 6, 8, 9, 10}) can_hit = can_hit || f[k] != 0.0f;
    recs[i].pad0 = can_hit ? c->bvh_tris[i].first : 0u;
    recs[i].pad1 = can_hit ? c->bvh_tris[i].second : 0u;
  }
  if (c->sample_textures) {
    for (uint32_t i = 0; i < need; ++i)
      for (uint32_t j = 0; j < i; ++j)
        if (recs[i].pad0 < recs[i].pad1 && recs[j].pad0 < recs[j].pad1 && recs[i].pad0 < recs[j].pad1 &&
            recs[j].pad0 < recs[i].pad1) {
          srt::SetError("texture sampling needs BVH records with disjoint triangle ranges");
          return SRT_ERR_INVALID;
        }
  }
  if (int rq = Quiesce(c)) return rq;
  if (need > c->bvh_capacity) {
    FreeDev(c->d_bvhs);
    c->d_bvhs = nullptr;
    HIP_OK(hipMalloc(&c->d_bvhs, sizeof(srt_bvh_record) * need));
    c->bvh_capacity = need;
  }
  HIP_OK(hipMemcpyAsync(c->d_bvhs, recs.data(), sizeof(srt_bvh_record) * need, hipMemcpyHostToDevice, c->stream));
  HIP_OK(hipStreamSynchronize(c->stream));
  c->bvh_uploaded = need;
  c->bvhs_dirty = false;
  return SRT_OK;
}

int EnsureLights(srt_context* c) {
  if (!c->lights_dirty) return SRT_OK;
  // the uploaded records plus one zero record that out-of-range indices map
  // to (lights[lightCount] is an out-of-bounds SSBO read, src/main.cpp:690)
  const size_t n = c->h_lights.size() + 1;
  std::vector<float4> rec(2 * n, make_float4(0, 0, 0, 0));
  for (size_t i = 0; i < c->h_lights.size(); ++i) {
    const srt_light& l = c->h_lights[i];
    rec[2 * i] = make_float4(l.position[0], l.position[1], l.position[2], l.intensity);
    rec[2 * i + 1] = make_float4(l.color[0], l.color[1], l.color[2], 0.0f);
  }
  if (int rq = Quiesce(c)) return rq;
  if (n > c->light_capacity) {
    FreeDev(c->d_lights);
    c->d_lights = nullptr;
    HIP_OK(hipMalloc(&c->d_lights, sizeof(float4) * 2 * n));
    c->light_capacity = (uint32_t)n;
  }
  HIP_OK(hipMemcpyAsync(c->d_lights, rec.data(), sizeof(float4) * 2 * n, hipMemcpyHostToDevice, c->stream));
  HIP_OK(hipStreamSynchronize(c->stream));
  c->lights_dirty = false;
  return SRT_OK;
}

int DetachImages(srt_context* c) {
  if (!c) return SRT_ERR_INVALID;
  HIP_OK(hipSetDevice(c->device));
  HIP_OK(hipStreamSynchronize(c->stream));
  if (int rq = Quiesce(c)) return rq;
  if (!c->images_external) { FreeDev(c->d_accum); FreeDev(c->d_out); }
  c->d_accum = nullptr;
  c->d_out = nullptr;
  c->images_external = false;
  c->img_w = c->img_rows = 0;
  c->rank = 0;
  c->nranks = 1;
  return SRT_OK;
}

}  // namespace srt

using srt::FreeDev, srt::LocalRows, srt::Quiesce, srt::SpanUnionMs;

// ===========================================================================
// C ABI (context part)
// ===========================================================================
extern "C" {

const char* srt_last_error(void) { return srt::LastError(); }
int srt_abi_version(void) { return SRT_ABI_VERSION; }

int srt_create(int device, void* stream, srt_context** out) {
  if (!out) return SRT_ERR_INVALID;
  HIP_OK(hipSetDevice(device));
  auto* c = new srt_context();
  c->device = device;
  if (const char* e = std::getenv("SRT_FORCE_GLOBAL_SCENE")) c->force_global = e[0] == '1';
  if (const char* e = std::getenv("SRT_SAMPLE_BUFFER_MB")) c->lbuf_total = (size_t)std::max(1L, std::atol(e)) << 20;
  if (const char* e = std::getenv("SRT_SAMPLE_BUFFER_KB")) c->lbuf_total = (size_t)std::max(1L, std::atol(e)) << 10;
  if (const char* e = std::getenv("SRT_BOUNCE_CAP")) c->bounce_cap = std::max(1, std::atoi(e));
  if (const char* e = std::getenv("SRT_POOL")) c->pool = e[0] == '1';
  if (const char* e = std::getenv("SRT_POOL_BATCH")) c->pool_batch = std::max(1, std::min(64, std::atoi(e)));
  if (const char* e = std::getenv("SRT_POOL_TLOW")) c->pool_tlow = std::max(1, std::atoi(e));
  if (const char* e = std::getenv("SRT_POOL_SLOTS")) c->pool_slots_max = std::max(64, std::atoi(e));
  if (const char* e = std::getenv("SRT_POOL_DEADLINE_MS")) c->pool_deadline_ms = std::max(1, std::atoi(e));
  if (const char* e = std::getenv("SRT_SPHERE_BLOCKS")) c->sphere_blocks = std::max(1, std::atoi(e));
  if (const char* e = std::getenv("SRT_WAVEFRONT")) c->wavefront = e[0] == '1' ? 1 : 0;
  if (const char* e = std::getenv("SRT_WF_SLOTS")) c->wf_slots = (uint32_t)std::max(256L, std::min(1L << 28, std::atol(e)));
  if (const char* e = std::getenv("SRT_WF_WAVES")) c->wf_waves = std::atoi(e);
  if (const char* e = std::getenv("SRT_TREELETS")) c->treelets = e[0] == '1' ? 1 : 0;
  if (const char* e = std::getenv("SRT_TREELET_DEPTH")) c->treelet_depth = std::max(0, std::min(srt::kTopStack - 1, std::atoi(e)));
  if (const char* e = std::getenv("SRT_PIPELINE")) c->pipe = std::max(1, std::min(8, std::atoi(e)));
  if (const char* e = std::getenv("SRT_PIPELINE_OVERLAP")) c->pipe_overlap = std::max(0, std::min(2, std::atoi(e)));
  if (const char* e = std::getenv("SRT_TAIL_CLAIMS"))
    c->tail_claims = c->tail_claims_sph = c->tail_claims_gw5 = std::max(0, std::atoi(e));
  if (const char* e = std::getenv("SRT_TILE_ORDER")) c->tile_schedule = e[0] != '0';
  if (const char* e = std::getenv("SRT_TILE_CULL")) c->tile_cull = e[0] != '0';
  if (const char* e = std::getenv("SRT_TILE_CULL_MIN_SAMPLES")) c->cull_min_samples = std::max(0LL, std::atoll(e));
  if (const char* e = std::getenv("SRT_TRAV_FRAC16")) c->trav_frac16 = std::max(0, std::min(16, std::atoi(e)));
  if (const char* e = std::getenv("SRT_TRAV_FRAC16_GLOBAL"))
    c->trav_frac16_global = std::max(0, std::min(16, std::atoi(e))), c->trav_frac16_global_env = true;
  {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0)
      c->num_cus = prop.multiProcessorCount;
  }
  if (stream) {
    c->stream = static_cast<hipStream_t>(stream);
  } else {
    hipError_t e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    if (e != hipSuccess) {
      delete c;
      srt::SetError(std::string("hipStreamCreate: ") + hipGetErrorString(e));
      return SRT_ERR_HIP;
    }
    c->own_stream = true;
  }
  c->lstream = c->stream;
  if (hipMalloc(&c->d_stats, sizeof(unsigned long long) * srt::ST_TOTAL) != hipSuccess ||
      hipMemset(c->d_stats, 0, sizeof(unsigned long long) * srt::ST_TOTAL) != hipSuccess ||
      hipMalloc(&c->d_nan, sizeof(unsigned long long)) != hipSuccess ||
      hipMemset(c->d_nan, 0, sizeof(unsigned long long)) != hipSuccess) {
    FreeDev(c->d_stats);
    FreeDev(c->d_nan);
    if (c->own_stream) (void)hipStreamDestroy(c->stream);
    delete c;
    srt::SetError("hipMalloc(stats) failed");
    return SRT_ERR_HIP;
  }
  *out = c;
  return SRT_OK;
}

int srt_destroy(srt_context* c) {
  if (!c) return SRT_ERR_INVALID;
  (void)hipSetDevice(c->device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  (void)Quiesce(c);
  for (auto& sl : c->slots) {
    FreeDev(sl.lbuf); FreeDev(sl.batch_ctr); FreeDev(sl.tile_cost); FreeDev(sl.tile_order); FreeDev(sl.gstack);
    if (sl.sampled) (void)hipEventDestroy(sl.sampled);
    if (sl.accumulated) (void)hipEventDestroy(sl.accumulated);
    if (sl.stream) (void)hipStreamDestroy(sl.stream);
  }
  c->slots.clear();
  if (c->plain_done) (void)hipEventDestroy(c->plain_done);
  FreeDev(c->d_nodes); FreeDev(c->d_tris); FreeDev(c->d_mats); FreeDev(c->d_bvhs); FreeDev(c->d_lights);
  FreeDev(c->d_tex); FreeDev(c->d_tex_info); FreeDev(c->d_tri_uv);
  FreeDev(c->d_noise_xy); FreeDev(c->d_noise_u); FreeDev(c->d_stats); FreeDev(c->d_nan); FreeDev(c->d_lbuf); FreeDev(c->d_gstack);
  FreeDev(c->d_batch_ctr); FreeDev(c->d_tile_cost); FreeDev(c->d_tile_order); FreeDev(c->d_row_map); FreeDev(c->d_span);
  for (auto& e : c->cull_ring) {
    FreeDev(e.d_live); FreeDev(e.d_sky);
    if (e.h_live) (void)hipHostFree(e.h_live);
    if (e.h_sky) (void)hipHostFree(e.h_sky);
    if (e.ready) (void)hipEventDestroy(e.ready);
    if (e.used) (void)hipEventDestroy(e.used);
  }
  if (c->cull_stream) (void)hipStreamDestroy(c->cull_stream);
  FreeDev(c->d_wf_rec); FreeDev(c->d_wf_res); FreeDev(c->d_wf_state); FreeDev(c->d_wf_rayq); FreeDev(c->d_wf_hitq);
  FreeDev(c->d_wf_ctl); FreeDev(c->d_wf_items);
  FreeDev(c->d_nodes_t); FreeDev(c->d_troot); FreeDev(c->d_tl_ray); FreeDev(c->d_tl_stk); FreeDev(c->d_tl_slist);
  FreeDev(c->d_tl_skey); FreeDev(c->d_tl_blist); FreeDev(c->d_tl_rlist); FreeDev(c->d_tl_count); FreeDev(c->d_tl_fill);
  if (c->h_wf_poll) (void)hipHostFree(c->h_wf_poll);
  for (hipEvent_t e : c->wf_poll_ev)
    if (e) (void)hipEventDestroy(e);
  for (hipEvent_t e : c->ev) (void)hipEventDestroy(e);
  if (!c->images_external) { FreeDev(c->d_accum); FreeDev(c->d_out); }
  if (c->own_stream) (void)hipStreamDestroy(c->stream);
  delete c;
  return SRT_OK;
}

void* srt_stream(srt_context* c) { return c ? static_cast<void*>(c->stream) : nullptr; }

int srt_set_bool(srt_context* c, const char* name, int v) {
  if (!c || !name) return SRT_ERR_INVALID;
  const std::string n(name);
  if (n == "resetAccumBuffer") c->reset = v ? 1 : 0;
  else if (n == "showModel") c->show_model = v ? 1 : 0;
  else return SRT_ERR_NOT_FOUND;
  return SRT_OK;
}

int srt_set_int(srt_context* c, const char* name, int v) {
  if (!c || !name) return SRT_ERR_INVALID;
  const std::string n(name);
  if (n == "Width") c->W = v;
  else if (n == "Height") c->H = v;
  else if (n == "accumFrames") c->accum_frames = v;
  else if (n == "lightCount") c->light_count = v;
  else if (n == "maxDepth") c->max_depth = v;
  else if (n == "resetAccumBuffer" || n == "showModel") return srt_set_bool(c, name, v);
  else if (n == "bvh_count") c->bvh_count = (uint32_t)v;
  else return SRT_ERR_NOT_FOUND;
  return SRT_OK;
}

int srt_set_uint(srt_context* c, const char* name, uint32_t v) {
  if (!c || !name) return SRT_ERR_INVALID;
  if (std::string(name) == "bvh_count") {
    c->bvh_count = v;
    return SRT_OK;
  }
  return srt_set_int(c, name, (int)v);
}

int srt_set_float(srt_context* c, const char* name, float v) {
  if (!c || !name) return SRT_ERR_INVALID;
  (void)v;
  return SRT_ERR_NOT_FOUND;  // the kernel declares no float uniforms
}

int srt_set_vec3(srt_context* c, const char* name, float x, float y, float z) {
  if (!c || !name) return SRT_ERR_INVALID;
  const std::string n(name);
  float* dst = nullptr;
  if (n == "cameraOrigin") dst = c->cam_origin;
  else if (n == "cameraDirection") dst = c->cam_dir;
  else if (n == "cameraUp") dst = c->cam_up;
  else if (n == "cameraRight") dst = c->cam_right;
  else return SRT_ERR_NOT_FOUND;
  dst[0] = x; dst[1] = y; dst[2] = z;
  return SRT_OK;
}

int srt_set_tiling(srt_context* c, int rank, int nranks, int band_rows) {
  if (!c || nranks < 1 || rank < 0 || rank >= nranks || band_rows < 1) return SRT_ERR_INVALID;
  c->rank = rank;
  c->nranks = nranks;
  c->band_rows = band_rows;
  return SRT_OK;
}

int srt_local_rows(srt_context* c) { return c ? LocalRows(c, c->H) : -1; }

int srt_device(srt_context* c) { return c ? c->device : -1; }

int srt_get_int(srt_context* c, const char* name, int* v) {
  if (!c || !name || !v) return SRT_ERR_INVALID;
  const std::string n(name);
  if (n == "Width") *v = c->W;
  else if (n == "Height") *v = c->H;
  else if (n == "accumFrames") *v = c->accum_frames;
  else if (n == "lightCount") *v = c->light_count;
  else if (n == "maxDepth") *v = c->max_depth;
  else if (n == "bvh_count") *v = (int)c->bvh_count;
  else if (n == "resetAccumBuffer") *v = c->reset;
  else if (n == "showModel") *v = c->show_model;
  else if (n == "scene.fused") *v = c->fused ? 1 : 0;
  else if (n == "scene.top_depth") *v = c->top_depth;  // levels in the fused instance's LDS copy (0: none)
  else if (n == "scene.top_f4") *v = c->top_f4;
  else if (n == "launch.top_f4") *v = c->launch_top_f4;
  else if (n == "scene.global_waves") *v = c->global_waves;
  else if (n == "scene.wavefront") *v = c->wavefront >= 0 ? c->wavefront : (c->wf_scene ? 1 : 0);
  else if (n == "scene.wf_waves") *v = c->wf_waves;
  else if (n == "scene.treelets") *v = (int)c->n_treelets;
  else if (n == "scene.tri_slots") *v = (int)c->n_tris;  // device triangle records (LayoutTris gaps included)
  else if (n == "launch.chunks") *v = c->ev_used / 2;   // sample launches of the last render or dispatch
  else if (n == "launch.overlap") *v = c->launch_overlap ? 1 : 0;  // what the last render's launches did
  else if (n == "launch.blocks_per_cu") *v = c->launch_per_cu;      // resident blocks per CU of the last sample launch
  else if (n == "launch.block") *v = c->launch_block;               // its lanes per block
  else if (n == "launch.mats_lds") *v = c->launch_mats_lds;          // 1: it read the material records from LDS
  else if (n == "launch.live_tiles") *v = c->launch_live_tiles;      // tiles its launches traced (tile_cull.hpp)
  else if (n == "cull.uploads") *v = (int)std::min<unsigned long long>(c->cull_uploads, 0x7FFFFFFF);  // maps sent to the device
  else if (n == "launch.culled_samples")                             // samples the last render did not trace
    *v = (int)std::min<long long>(c->launch_culled, 0x7FFFFFFF);
  else return SRT_ERR_NOT_FOUND;
  return SRT_OK;
}

// Kernel time of sample launches: the union of their span records (scene_layout.cpp SpanUnionMs).
int srt_last_kernel_ms(srt_context* c, float* ms) {
  if (!c || !ms) return SRT_ERR_INVALID;
  *ms = 0.0f;
  std::vector<unsigned long long> ring;
  unsigned long long lo = ~0ull, hi = 0;  // the render's span records (its chunks' launches are consecutive)
  for (int i = 0; i + 1 < c->ev_used; i += 2) {
    HIP_OK(hipEventSynchronize(c->ev[i + 1]));
    const size_t chunk = (size_t)(i / 2);
    const long long rec = chunk < c->chunk_span.size() ? c->chunk_span[chunk] : -1;
    if (rec >= 0 && (unsigned long long)rec + srt_context::kSpanCap >= c->span_seq) {  // the launch's own span
      lo = std::min(lo, (unsigned long long)rec);
      hi = std::max(hi, (unsigned long long)rec + 1);
      continue;
    }
    float t = 0.0f;  // pool and wavefront launches: the HIP events around them
    HIP_OK(hipEventElapsedTime(&t, c->ev[i], c->ev[i + 1]));
    *ms += t;
  }
  if (lo < hi) {
    ring.resize(2 * srt_context::kSpanCap);
    HIP_OK(hipMemcpy(ring.data(), c->d_span, sizeof(unsigned long long) * ring.size(), hipMemcpyDeviceToHost));
    *ms += (float)SpanUnionMs(ring.data(), c->span_seq, srt_context::kSpanCap, lo, hi, 0ull, nullptr);
  }
  return SRT_OK;
}

int srt_kernel_time(srt_context* c, double* total_ms, int* launches) {
  if (!c || !total_ms || !launches) return SRT_ERR_INVALID;
  *total_ms = 0.0;
  *launches = 0;
  HIP_OK(hipStreamSynchronize(c->stream));
  if (int rq = Quiesce(c)) return rq;
  const unsigned long long from = c->span_read;
  c->span_read = c->span_seq;
  if (c->span_seq - from > (unsigned long long)srt_context::kSpanCap) {  // records were overwritten unread
    srt::SetError("srt_kernel_time: more than 4096 sample launches since the last call (span records lost)");
    return SRT_ERR_LIMIT;
  }
  if (c->span_seq > from) {
    std::vector<unsigned long long> ring(2 * srt_context::kSpanCap);
    HIP_OK(hipMemcpy(ring.data(), c->d_span, sizeof(unsigned long long) * ring.size(), hipMemcpyDeviceToHost));
    // (time before the end of the launches read by the previous call was counted there)
    *total_ms = SpanUnionMs(ring.data(), c->span_seq, srt_context::kSpanCap, from, c->span_seq, c->span_done,
                            &c->span_done);
    *launches = (int)(c->span_seq - from);
  }
  return SRT_OK;
}

int srt_get_stats(srt_context* c, srt_stats* out) {
  if (!c || !out) return SRT_ERR_INVALID;
  *out = c->stats;
  return SRT_OK;
}

int srt_ray_kinds(srt_context* c, uint64_t kinds[3]) {
  if (!c || !kinds) return SRT_ERR_INVALID;
  kinds[0] = c->stats.samples;  // one camera ray per path sample
  kinds[1] = c->shadow_rays;
  kinds[2] = c->stats.rays - c->stats.samples - c->shadow_rays;
  return SRT_OK;
}

int srt_reset_stats(srt_context* c) {
  if (!c) return SRT_ERR_INVALID;
  c->stats = srt_stats{};
  c->shadow_rays = 0;
  HIP_OK(hipSetDevice(c->device));
  HIP_OK(hipMemsetAsync(c->d_nan, 0, sizeof(unsigned long long), c->stream));
  HIP_OK(hipStreamSynchronize(c->stream));
  return SRT_OK;
}

int srt_nan_samples(srt_context* c, uint64_t* out) {
  if (!c || !out) return SRT_ERR_INVALID;
  unsigned long long v = 0;
  HIP_OK(hipSetDevice(c->device));
  HIP_OK(hipMemcpyAsync(&v, c->d_nan, sizeof(v), hipMemcpyDeviceToHost, c->stream));
  HIP_OK(hipStreamSynchronize(c->stream));
  *out = v;
  return SRT_OK;
}

int srt_set_lights(srt_context* c, const srt_light* lights, uint32_t n) {
  if (!c || (n && !lights)) return SRT_ERR_INVALID;
  c->h_lights.assign(lights, lights + n);
  c->lights_dirty = true;
  return SRT_OK;
}

int srt_set_noise(srt_context* c, const float* noise_rgb, const float* noise_u_rgb, size_t texels) {
  if (!c || !noise_rgb || !noise_u_rgb || texels == 0) return SRT_ERR_INVALID;
  HIP_OK(hipSetDevice(c->device));
  if (int rq = Quiesce(c)) return rq;
  std::vector<float2> xy(texels);
  std::vector<float> u(texels);
  // (and the exact extremes of the jitter, which bound every sample's place in its pixel: tile_cull.hpp)
  float mn[2] = {noise_rgb[0], noise_rgb[1]}, mx[2] = {noise_rgb[0], noise_rgb[1]};
  bool finite = true;
  for (size_t i = 0; i < texels; ++i) {
    xy[i] = make_float2(noise_rgb[3 * i], noise_rgb[3 * i + 1]);
    u[i] = noise_u_rgb[3 * i];
    for (int k = 0; k < 2; ++k) {
      const float v = noise_rgb[3 * i + k];
      finite = finite && std::isfinite(v);
      mn[k] = std::min(mn[k], v);
      mx[k] = std::max(mx[k], v);
    }
  }
  c->noise_finite = false;  // (until the upload below has succeeded)
  ++c->cull_gen;
  if (texels != c->noise_texels) {
    FreeDev(c->d_noise_xy); FreeDev(c->d_noise_u);
    c->d_noise_xy = nullptr; c->d_noise_u = nullptr; c->noise_texels = 0;
    HIP_OK(hipMalloc(&c->d_noise_xy, texels * sizeof(float2)));
    HIP_OK(hipMalloc(&c->d_noise_u, texels * sizeof(float)));
  }
  HIP_OK(hipMemcpyAsync(c->d_noise_xy, xy.data(), texels * sizeof(float2), hipMemcpyHostToDevice, c->stream));
  HIP_OK(hipMemcpyAsync(c->d_noise_u, u.data(), texels * sizeof(float), hipMemcpyHostToDevice, c->stream));
  HIP_OK(hipStreamSynchronize(c->stream));
  c->noise_texels = texels;
  for (int k = 0; k < 2; ++k) c->nz_min[k] = mn[k], c->nz_max[k] = mx[k];
  c->noise_finite = finite;
  return SRT_OK;
}

int srt_alloc_images(srt_context* c) {
  if (!c || c->W <= 0 || c->H <= 0) return SRT_ERR_STATE;
  HIP_OK(hipSetDevice(c->device));
  const int rows = LocalRows(c, c->H);
  const size_t px = (size_t)c->W * (size_t)std::max(rows, 1);
  if (!c->images_external) { FreeDev(c->d_accum); FreeDev(c->d_out); }
  c->images_external = false;
  c->d_accum = nullptr; c->d_out = nullptr;
  HIP_OK(hipMalloc(&c->d_accum, px * sizeof(float4)));
  HIP_OK(hipMalloc(&c->d_out, px * sizeof(uint32_t)));
  HIP_OK(hipMemsetAsync(c->d_accum, 0, px * sizeof(float4), c->stream));
  HIP_OK(hipMemsetAsync(c->d_out, 0, px * sizeof(uint32_t), c->stream));
  HIP_OK(hipStreamSynchronize(c->stream));
  c->img_w = c->W;
  c->img_rows = rows;
  return SRT_OK;
}

int srt_read_accum(srt_context* c, float* host, size_t bytes) {
  if (!c || !host || !c->d_accum) return SRT_ERR_INVALID;
  const size_t need = (size_t)c->img_w * c->img_rows * sizeof(float4);
  if (bytes < need) return SRT_ERR_INVALID;
  HIP_OK(hipMemcpyAsync(host, c->d_accum, need, hipMemcpyDeviceToHost, c->stream));
  HIP_OK(hipStreamSynchronize(c->stream));
  return SRT_OK;
}

int srt_write_accum(srt_context* c, const float* host, size_t bytes) {
  if (!c || !host || !c->d_accum) return SRT_ERR_INVALID;
  const size_t need = (size_t)c->img_w * c->img_rows * sizeof(float4);
  if (bytes < need) return SRT_ERR_INVALID;
  HIP_OK(hipMemcpyAsync(c->d_accum, host, need, hipMemcpyHostToDevice, c->stream));
  HIP_OK(hipStreamSynchronize(c->stream));
  return SRT_OK;
}

namespace {
constexpr char kCkptMagic[8] = {'S', 'R', 'T', 'C', 'K', 'P', 'T', '1'};
struct CkptHeader {
  char magic[8];
  int32_t version, width, local_rows, rank, nranks, band_rows, accum_frames, pad;
  float cam[12];  // cameraOrigin, cameraDirection, cameraUp, cameraRight
  uint64_t payload_bytes;
  uint32_t payload_crc, header_crc;
};
uint32_t Crc32(const void* p, size_t n) {
  return (uint32_t)crc32(0L, static_cast<const Bytef*>(p), (uInt)n);
}
}  // namespace

int srt_checkpoint_save(srt_context* c, const char* path) {
  if (!c || !path || !c->d_accum || c->img_w <= 0 || c->img_rows <= 0) return SRT_ERR_INVALID;
  std::vector<float> acc((size_t)c->img_w * c->img_rows * 4);
  int rc = srt_read_accum(c, acc.data(), acc.size() * sizeof(float));
  if (rc) return rc;
  CkptHeader h{};
  std::memcpy(h.magic, kCkptMagic, 8);
  h.version = 1;
  h.width = c->img_w;
  h.local_rows = c->img_rows;
  h.rank = c->rank;
  h.nranks = c->nranks;
  h.band_rows = c->band_rows;
  h.accum_frames = c->accum_frames;
  const float* cam[4] = {c->cam_origin, c->cam_dir, c->cam_up, c->cam_right};
  for (int i = 0; i < 4; ++i) std::memcpy(h.cam + 3 * i, cam[i], 3 * sizeof(float));
  h.payload_bytes = acc.size() * sizeof(float);
  h.payload_crc = Crc32(acc.data(), h.payload_bytes);
  h.header_crc = Crc32(&h, offsetof(CkptHeader, header_crc));
  const std::string tmp = std::string(path) + ".tmp";
  FILE* f = std::fopen(tmp.c_str(), "wb");
  if (!f) {
    srt::SetError(std::string("srt_checkpoint_save: cannot open ") + tmp);
    return SRT_ERR_IO;
  }
  const bool ok = std::fwrite(&h, sizeof h, 1, f) == 1 && std::fwrite(acc.data(), 1, h.payload_bytes, f) == h.payload_bytes;
  if (std::fclose(f) != 0 || !ok || std::rename(tmp.c_str(), path) != 0) {  // the old file survives a failed save
    std::remove(tmp.c_str());
    srt::SetError(std::string("srt_checkpoint_save: cannot write ") + path);
    return SRT_ERR_IO;
  }
  return SRT_OK;
}

int srt_checkpoint_load(srt_context* c, const char* path, int32_t* accum_frames) {
  if (!c || !path || !c->d_accum) return SRT_ERR_INVALID;
  FILE* f = std::fopen(path, "rb");
  if (!f) {
    srt::SetError(std::string("srt_checkpoint_load: cannot open ") + path);
    return SRT_ERR_IO;
  }
  CkptHeader h{};
  std::vector<float> acc;
  bool ok = std::fread(&h, sizeof h, 1, f) == 1 && std::memcmp(h.magic, kCkptMagic, 8) == 0 && h.version == 1 &&
            h.header_crc == Crc32(&h, offsetof(CkptHeader, header_crc));
  if (ok && (h.width != c->img_w || h.local_rows != c->img_rows || h.rank != c->rank || h.nranks != c->nranks ||
             h.band_rows != c->band_rows || h.payload_bytes != (uint64_t)c->img_w * c->img_rows * 16)) {
    std::fclose(f);
    srt::SetError("srt_checkpoint_load: the checkpoint's frame or tiling differs from the context's");
    return SRT_ERR_INVALID;
  }
  if (ok) {
    acc.resize(h.payload_bytes / sizeof(float));
    ok = std::fread(acc.data(), 1, h.payload_bytes, f) == h.payload_bytes &&
         Crc32(acc.data(), h.payload_bytes) == h.payload_crc;
  }
  std::fclose(f);
  if (!ok) {
    srt::SetError(std::string("srt_checkpoint_load: not a valid checkpoint (truncated or corrupt): ") + path);
    return SRT_ERR_IO;
  }
  const int rc = srt_write_accum(c, acc.data(), h.payload_bytes);
  if (rc) return rc;
  c->accum_frames = h.accum_frames;
  float* cam[4] = {c->cam_origin, c->cam_dir, c->cam_up, c->cam_right};
  for (int i = 0; i < 4; ++i) std::memcpy(cam[i], h.cam + 3 * i, 3 * sizeof(float));
  if (accum_frames) *accum_frames = h.accum_frames;
  return SRT_OK;
}

int srt_read_output(srt_context* c, uint8_t* host, size_t bytes) {
  if (!c || !host || !c->d_out) return SRT_ERR_INVALID;
  const size_t need = (size_t)c->img_w * c->img_rows * sizeof(uint32_t);
  if (bytes < need) return SRT_ERR_INVALID;
  HIP_OK(hipMemcpyAsync(host, c->d_out, need, hipMemcpyDeviceToHost, c->stream));
  HIP_OK(hipStreamSynchronize(c->stream));
  return SRT_OK;
}

int srt_write_output(srt_context* c, const char* path, int flip_y) {
  if (!c || !path || !c->d_out || c->img_w <= 0 || c->img_rows <= 0) return SRT_ERR_INVALID;
  std::vector<uint8_t> px((size_t)c->img_w * c->img_rows * 4);
  const int rc = srt_read_output(c, px.data(), px.size());
  if (rc) return rc;
  return srt_image_write(path, px.data(), c->img_w, c->img_rows, flip_y);
}

int srt_set_image_buffers(srt_context* c, void* accum_dev, void* out_dev) {
  if (!c || !accum_dev || !out_dev || c->W <= 0 || c->H <= 0) return SRT_ERR_INVALID;
  if (!c->images_external) { FreeDev(c->d_accum); FreeDev(c->d_out); }
  c->d_accum = static_cast<float4*>(accum_dev);
  c->d_out = static_cast<uint32_t*>(out_dev);
  c->images_external = true;
  c->img_w = c->W;
  c->img_rows = LocalRows(c, c->H);
  return SRT_OK;
}

int srt_assemble_bands(srt_context* c, const void* gathered, int nranks, int rows_pad, int band_rows, int frames,
                       void* accum_full, void* out_full) {
  return c ? srt::AssembleBandsOn(c, c->stream, gathered, nranks, rows_pad, band_rows, frames, accum_full, out_full)
           : SRT_ERR_INVALID;
}

int srt_assemble_output_bands(srt_context* c, const void* gathered_rgba8, int nranks, int rows_pad, int band_rows,
                              void* out_full) {
  return c ? srt::AssembleOutputOn(c, c->stream, gathered_rgba8, nranks, rows_pad, band_rows, c->W, c->H, out_full)
           : SRT_ERR_INVALID;
}

int srt_image_pointers(srt_context* c, void** accum_dev, void** out_dev) {
  if (!c) return SRT_ERR_INVALID;
  if (accum_dev) *accum_dev = c->d_accum;
  if (out_dev) *out_dev = c->d_out;
  return SRT_OK;
}

}  // extern "C"
