// scene_refit.hip -- the path tracer's scene refit (include/srt_scene_refit.h): the object an upload hands out,
// the launches of refit_kernels.hpp's kernels on the context's stream, and the readback of a context's device
// scene.  A translation unit of its own beside pathtrace.hip, which it only reads: the context's fields through
// context.hpp, the device constants through traversal.hpp.  pathtrace.hip and its headers (the device code
// srt_code_hash identifies) are unchanged.
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "../../include/srt_scene_refit.h"
#include "capi_objects.hpp"
#include "context.hpp"
#include "launch_plan.hpp"
#include "scene_image_maps.hpp"
#include "scene_layout.hpp"
#include "scene_refit.hpp"
#include "scene_refit_host.hpp"
#include "stage.hpp"
#include "traversal.hpp"

// The values pathtrace.hip's kBuild holds, for the one use BuildSceneImage makes of them.  The constants come
// from the device header; the three macros whose defaults pathtrace.hip and kernels.hpp set (kernels.hpp defines
// kernels, so only one unit may include it) are restated with the same defaults -- an experiment build sets them on
// the hipcc line, which this unit shares.  tests/test_scene_refit_api.py holds the copies to the originals; and
// should the two ever disagree at run time, the layout recomputed here is compared with the uploaded one (sizes,
// top region, roots, triangle ranges) and srt_upload_scene_refit answers SRT_ERR_STATE.
#ifndef SRT_LDS_BLOCK
#define SRT_LDS_BLOCK 1024
#endif
#ifndef SRT_GW5_BLOCK
#define SRT_GW5_BLOCK 256
#endif
#ifndef SRT_RING_GW5
#define SRT_RING_GW5 8
#endif

struct srt_scene_refit {
  srt_context* ctx = nullptr;
  // the context's arrays and counts at creation: what a refit compares before it writes
  float4 *d_nodes = nullptr, *d_nodes_t = nullptr, *d_tris = nullptr;
  uint32_t n_nodes = 0, n_tslots = 0, ref_or = 0;
  int top_f4 = 0;
  uint32_t n_verts = 0, n_tris = 0, n_entries = 0;
  srt::stage::DevPtr<uint4> d_triples;
  srt::stage::DevPtr<uint32_t> d_schedule;  // n_entries (slot, triangle) pairs, then the tail's offsets
  srt::scene_refit::Schedule schedule;      // (order released: it lives on the device)
  hipEvent_t done = nullptr;
  std::vector<float4> h_roots;              // READ_ROOTS: 2 float4 per record
  size_t bytes = 0;
  unsigned long long count = 0;
};

namespace {

constexpr int RingOf(int gw) { return (gw > 4 || SRT_COOP) ? SRT_RING_GW5 : srt::kShortStack; }
// (lds_block and pool_trav_lanes size a launch, not the image; pool.hpp, which holds the latter, defines kernels)
constexpr srt::BuildConsts kBuild = {SRT_LDS_BLOCK, SRT_GW5_BLOCK, srt::kNodeBlkF4, RingOf(4), RingOf(5),
                                     SRT_COOP != 0, srt::kCoopWaveBytes, srt::kCoopIdxBits, 0,
                                     srt::kNodePad, (uint32_t)srt::kTriPad, srt::kTreeletCnt};

uint32_t AsUint(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  return u;
}

// The records' roots in the device layout: what LayoutNodes made of them at the upload and here.
bool SameRoots(const std::vector<srt_bvh_record>& a, const std::vector<srt_bvh_record>& b) {
  for (size_t i = 0; i < a.size() && i < b.size(); ++i)
    if (a[i].first_index != b[i].first_index) return false;
  return a.size() == b.size();
}

size_t NodesBytes(const srt_context* c) { return sizeof(float4) * 2 * ((size_t)c->n_nodes + 1); }
size_t TrisBytes(const srt_context* c) { return sizeof(float4) * 3 * ((size_t)c->n_tris + srt::kTriPad); }

int Attach(srt_context* c, const srt_bvh_record* bvhs, uint32_t n_bvhs, const srt_bvh_node* nodes, uint32_t n_nodes,
           const srt_material_obj* mats, const float* tex_albedo, uint32_t n_mats, const srt_triangle* tris,
           uint32_t n_tris, const srt_vertex* verts, uint32_t n_verts, struct srt_scene_refit* r) {
  static_assert(sizeof(srt::scene_refit::Entry) == sizeof(uint2), "the schedule is uploaded as it is");
  // the image again, from what the upload read: the same inputs, the same choices, now with the maps
  int depth = 0;
  std::vector<std::pair<uint32_t, uint32_t>> tri_ranges;
  std::vector<uint8_t> reach;
  if (int rc = srt::ValidateNodes(nodes, n_nodes, n_tris, bvhs, n_bvhs, &depth, &tri_ranges, &reach)) return rc;
  const srt::ScenePolicy policy = srt::ChooseScenePolicy(n_nodes, n_tris, c->treelet_depth, c->treelets);
  const srt::SceneArrays in{bvhs, n_bvhs, nodes, n_nodes, mats, tex_albedo, n_mats, tris, n_tris, verts, n_verts};
  srt::SceneImage img;
  srt::SceneMaps maps;
  srt::BuildSceneImageMaps(in, depth, std::move(tri_ranges), reach, policy, kBuild, c->h_lights.size(), &img, &maps);
  const int top_f4 = img.n_top > 0 ? 2 * (int)img.n_top + 2 : 0;
  if (c->n_nodes != img.n_slots + srt::kNodePad || c->n_tris != img.n_tslots || c->top_f4 != top_f4 ||
      c->ref_or != img.ref_or || (c->d_nodes_t != nullptr) != !img.nodes_t.empty() ||
      img.nodes.size() != 2 * ((size_t)c->n_nodes + 1) || c->top_depth != img.top_depth ||
      c->bvh_tris != img.bvh_tris || c->h_bvhs.size() != img.bvhs.size() || !SameRoots(c->h_bvhs, img.bvhs)) {
    srt::SetError("srt_upload_scene_refit: the layout recomputed for the refit differs from the uploaded one");
    return SRT_ERR_STATE;
  }
  // the schedule: every slot a record's root or slot 0 reaches, by height
  std::vector<uint32_t> ref(img.n_slots), cnt(img.n_slots), roots{0};
  for (uint32_t s = 0; s < img.n_slots; ++s) {
    ref[s] = AsUint(img.nodes[2 * (size_t)s + 2].w);
    cnt[s] = AsUint(img.nodes[2 * (size_t)s + 3].w);
  }
  for (const srt_bvh_record& b : img.bvhs) roots.push_back(b.first_index);
  std::vector<uint32_t> tri_of_slot(img.n_tslots, 0xFFFFFFFFu);
  for (uint32_t t = 0; t < n_tris; ++t)
    if (maps.tri_slot[t] < img.n_tslots) tri_of_slot[maps.tri_slot[t]] = t;
  srt::scene_refit::Schedule s;
  if (!srt::scene_refit::BuildSchedule(ref.data(), cnt.data(), img.n_slots, img.ref_or, roots.data(),
                                       (uint32_t)roots.size(), tri_of_slot.data(), img.n_tslots, n_tris, &s)) {
    srt::SetError("srt_upload_scene_refit: the device node records do not form the trees the upload validated");
    return SRT_ERR_STATE;
  }
  for (uint32_t t = 0; t < n_tris; ++t)
    if (maps.tri_slot[t] >= img.n_tslots) {
      srt::SetError("srt_upload_scene_refit: a triangle slot past the device array");
      return SRT_ERR_STATE;
    }
  const std::vector<uint32_t> triples = srt::scene_refit::BuildTriples(tris, n_tris, maps.tri_slot.data());
  std::vector<uint32_t> sched(2 * s.order.size());
  if (!s.order.empty()) std::memcpy(sched.data(), s.order.data(), sizeof(uint32_t) * sched.size());
  sched.insert(sched.end(), s.first.begin() + s.tail_begin, s.first.end());
  const size_t tb = triples.size() * sizeof(uint32_t), sb = sched.size() * sizeof(uint32_t);
  HIP_OK(hipSetDevice(c->device));
  HIP_OK(r->d_triples.Alloc(tb > 0 ? tb : 16));
  HIP_OK(r->d_schedule.Alloc(sb));
  if (tb) HIP_OK(hipMemcpyAsync(r->d_triples, triples.data(), tb, hipMemcpyHostToDevice, c->stream));
  HIP_OK(hipMemcpyAsync(r->d_schedule, sched.data(), sb, hipMemcpyHostToDevice, c->stream));
  HIP_OK(hipStreamSynchronize(c->stream));  // the host arrays go out of scope
  HIP_OK(hipEventCreateWithFlags(&r->done, hipEventDisableTiming));
  r->ctx = c;
  r->d_nodes = c->d_nodes;
  r->d_nodes_t = c->d_nodes_t;
  r->d_tris = c->d_tris;
  r->n_nodes = c->n_nodes;
  r->n_tslots = c->n_tris;
  r->ref_or = c->ref_or;
  r->top_f4 = c->top_f4;
  r->n_verts = n_verts;
  r->n_tris = n_tris;
  r->n_entries = (uint32_t)s.order.size();
  r->bytes = tb + sb;
  r->h_roots.assign(2 * c->h_bvhs.size(), make_float4(0, 0, 0, 0));
  s.order = std::vector<srt::scene_refit::Entry>();
  r->schedule = std::move(s);
  return SRT_OK;
}

void Free(struct srt_scene_refit* r) {
  if (r->ctx) (void)hipSetDevice(r->ctx->device);
  // the refits enqueued through the object have read its arrays before they go
  if (r->done) {
    (void)hipEventSynchronize(r->done);
    (void)hipEventDestroy(r->done);
  }
  delete r;
}

}  // namespace

extern "C" {

int srt_scene_refit_abi_version(void) { return SRT_SCENE_REFIT_ABI_VERSION; }

int srt_upload_scene_refit(srt_context* c, const srt_bvh_record* bvhs, uint32_t n_bvhs, const srt_bvh_node* nodes,
                           uint32_t n_nodes, const srt_material_obj* mats, const float* tex_albedo, uint32_t n_mats,
                           const srt_triangle* tris, uint32_t n_tris, const srt_vertex* verts, uint32_t n_verts,
                           struct srt_scene_refit** out) {
  if (out) *out = nullptr;
  if (!c || !out) return SRT_ERR_INVALID;
  int rc = srt_upload_scene(c, bvhs, n_bvhs, nodes, n_nodes, mats, tex_albedo, n_mats, tris, n_tris, verts, n_verts);
  if (rc) return rc;
  struct srt_scene_refit* r = new struct srt_scene_refit;
  rc = Attach(c, bvhs, n_bvhs, nodes, n_nodes, mats, tex_albedo, n_mats, tris, n_tris, verts, n_verts, r);
  if (rc) {
    Free(r);
    return rc;
  }
  *out = r;
  return SRT_OK;
}

// srt_upload_scene_obj's steps, with the upload that hands out the object
int srt_upload_scene_obj_refit(srt_context* c, const srt_scene* s, struct srt_scene_refit** out) {
  if (out) *out = nullptr;
  if (!c || !s || !out) return SRT_ERR_INVALID;
  const srt::Scene& sc = *s->s;
  if (sc.sample_textures) {
    std::vector<srt_texture> tx;
    for (const auto& t : sc.textures) tx.push_back(srt_texture{t.texels.data(), t.width, t.height, t.channels});
    const int rc = srt_upload_textures(c, tx.data(), (uint32_t)tx.size());
    if (rc) return rc;
  }
  return srt_upload_scene_refit(c, sc.bvhs.data(), (uint32_t)sc.bvhs.size(), sc.nodes.data(), (uint32_t)sc.nodes.size(),
                                sc.mats.data(), sc.sample_textures ? nullptr : sc.tex_albedo.data(),
                                (uint32_t)sc.mats.size(), sc.tris.data(), (uint32_t)sc.tris.size(), sc.verts.data(),
                                (uint32_t)sc.verts.size(), out);
}

int srt_scene_refit_destroy(struct srt_scene_refit* r) {
  if (!r) return SRT_ERR_INVALID;
  Free(r);
  return SRT_OK;
}

int srt_scene_refit(struct srt_scene_refit* r, const srt_vertex* verts_dev, uint32_t n_verts, uint32_t flags) {
  if (!r) return SRT_ERR_INVALID;
  if (!verts_dev || !srt::stage::Aligned(verts_dev, 16)) {
    srt::SetError("srt_scene_refit: verts_dev must be a 16-byte aligned device pointer");
    return SRT_ERR_INVALID;
  }
  if (n_verts != r->n_verts) {
    srt::SetError("srt_scene_refit: n_verts differs from the count at upload");
    return SRT_ERR_INVALID;
  }
  if (flags & ~SRT_SCENE_REFIT_READ_ROOTS) {
    srt::SetError("srt_scene_refit: unknown flag bits");
    return SRT_ERR_INVALID;
  }
  srt_context* c = r->ctx;
  if (!c->scene_ok || c->d_nodes != r->d_nodes || c->d_nodes_t != r->d_nodes_t || c->d_tris != r->d_tris ||
      c->n_nodes != r->n_nodes || c->n_tris != r->n_tslots || c->ref_or != r->ref_or || c->top_f4 != r->top_f4 ||
      2 * c->h_bvhs.size() != r->h_roots.size()) {
    srt::SetError("srt_scene_refit: the context's scene is no longer the one the object was made for");
    return SRT_ERR_STATE;
  }
  HIP_OK(hipSetDevice(c->device));
  if (int rq = srt::Quiesce(c)) return rq;  // pipelined launches still read the old boxes
  srt::scene_refit::SParams sp;
  std::memset(&sp, 0, sizeof sp);
  sp.nodes = c->d_nodes;
  sp.nodes_t = c->d_nodes_t;
  sp.tris = c->d_tris;
  sp.triples = r->d_triples;
  sp.order = reinterpret_cast<const uint2*>(r->d_schedule.get());
  sp.tail_first = r->d_schedule + 2 * (size_t)r->n_entries;
  sp.verts = reinterpret_cast<const float4*>(verts_dev);
  sp.n_verts = n_verts;
  sp.n_tris = r->n_tris;
  sp.ref_or = c->ref_or;
  if (int rc = srt::refit::Enqueue<srt::scene_refit::SlotLayout>(c->stream, sp, r->schedule)) return rc;
  // every stream the context launches on waits for the refit (a slot's launch otherwise waits only for that
  // slot's last accumulation)
  HIP_OK(hipEventRecord(r->done, c->stream));
  for (auto& sl : c->slots)
    if (sl.stream) HIP_OK(hipStreamWaitEvent(sl.stream, r->done, 0));
  HIP_OK(hipStreamWaitEvent(c->stream, r->done, 0));
  // The slots' streams are created by the context's first pipelined launch, and a new slot's first launch waits
  // for nothing on `stream`: before they exist there is no stream to hand the event to, so the call waits for its
  // own kernels this once (the first frame of a context; every later refit only enqueues).
  if (c->pipe > 1 && c->slots.empty()) HIP_OK(hipStreamSynchronize(c->stream));
  ++r->count;
  // tile culling reads the host copies of the root boxes (tile_cull.hpp)
  c->roots_ok = false;
  ++c->cull_gen;
  if (flags & SRT_SCENE_REFIT_READ_ROOTS) {
    bool ok = true;
    for (size_t i = 0; i < c->h_bvhs.size(); ++i) {
      const size_t at = 2 * (size_t)c->h_bvhs[i].first_index + 2;
      if (at + 2 > 2 * ((size_t)c->n_nodes + 1)) {  // no box to read, as at upload: culling stays off
        ok = false;
        break;
      }
      HIP_OK(hipMemcpyAsync(&r->h_roots[2 * i], c->d_nodes + at, 2 * sizeof(float4), hipMemcpyDeviceToHost, c->stream));
    }
    HIP_OK(hipStreamSynchronize(c->stream));
    if (ok) {
      for (size_t i = 0; i < c->h_bvhs.size(); ++i) {
        const float4 lo = r->h_roots[2 * i], hi = r->h_roots[2 * i + 1];
        c->h_roots[i] = srt::RootBox{{lo.x, lo.y, lo.z}, {hi.x, hi.y, hi.z}};
      }
      c->roots_ok = true;
    }
  }
  return SRT_OK;
}

int srt_scene_refit_get_int(struct srt_scene_refit* r, const char* name, int* v) {
  if (!r || !name || !v) return SRT_ERR_INVALID;
  const std::string n(name);
  if (n == "refit.launches") *v = (int)r->schedule.launches;
  else if (n == "refit.heights") *v = (int)r->schedule.heights;
  else if (n == "refit.count") *v = (int)r->count;
  else if (n == "refit.bytes") *v = r->bytes > 0x7FFFFFFFu ? 0x7FFFFFFF : (int)r->bytes;  // (saturates at INT_MAX)
  else if (n == "refit.treelets") *v = r->d_nodes_t ? 1 : 0;
  else return SRT_ERR_NOT_FOUND;
  return SRT_OK;
}

int srt_scene_device_bytes(srt_context* c, size_t bytes[3]) {
  if (!c || !bytes) return SRT_ERR_INVALID;
  if (!c->scene_ok) { srt::SetError("no scene uploaded"); return SRT_ERR_STATE; }
  bytes[0] = NodesBytes(c);
  bytes[1] = c->d_nodes_t ? NodesBytes(c) : 0;
  bytes[2] = TrisBytes(c);
  return SRT_OK;
}

int srt_scene_copy_device(srt_context* c, void* nodes, void* nodes_t, void* tris) {
  if (!c) return SRT_ERR_INVALID;
  if (!c->scene_ok) { srt::SetError("no scene uploaded"); return SRT_ERR_STATE; }
  HIP_OK(hipSetDevice(c->device));
  if (int rq = srt::Quiesce(c)) return rq;
  HIP_OK(hipStreamSynchronize(c->stream));
  if (nodes) HIP_OK(hipMemcpy(nodes, c->d_nodes, NodesBytes(c), hipMemcpyDeviceToHost));
  if (nodes_t && c->d_nodes_t) HIP_OK(hipMemcpy(nodes_t, c->d_nodes_t, NodesBytes(c), hipMemcpyDeviceToHost));
  if (tris) HIP_OK(hipMemcpy(tris, c->d_tris, TrisBytes(c), hipMemcpyDeviceToHost));
  return SRT_OK;
}

}  // extern "C"
