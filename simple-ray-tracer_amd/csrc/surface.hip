// surface.hip -- the surface-attribute stage of include/srt_surface.h: a device copy of the scene in
// surface_host.hpp's layout, the textures, and the launch of surface_shade_kernel (surface.hpp).  A translation
// unit of its own, as query.hip is: pathtrace.hip and its headers (the device code srt_code_hash identifies) are
// only read.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/srt_surface.h"
#include "surface.hpp"
#include "surface_host.hpp"

#define SHIP_OK(expr)                                                         \
  do {                                                                        \
    hipError_t e_ = (expr);                                                   \
    if (e_ != hipSuccess) {                                                   \
      srt::SetError(std::string(#expr) + ": " + hipGetErrorString(e_));       \
      return SRT_ERR_HIP;                                                     \
    }                                                                         \
  } while (0)

struct srt_surface {
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  float* d_frames = nullptr;
  float4* d_tris = nullptr;
  float4* d_mats = nullptr;
  uint32_t* d_texels = nullptr;
  uint4* d_tex_info = nullptr;
  uint32_t n_bvhs = 0, bvh_count = 0, n_tris = 0, n_tex = 0;
  int last_blocks = 0;
};

namespace {

using srt::surface::kBlock;
using srt::surface::SParams;

void FreeAll(srt_surface* s) {
  if (s->d_frames) (void)hipFree(s->d_frames);
  if (s->d_tris) (void)hipFree(s->d_tris);
  if (s->d_mats) (void)hipFree(s->d_mats);
  if (s->d_texels) (void)hipFree(s->d_texels);
  if (s->d_tex_info) (void)hipFree(s->d_tex_info);
  if (s->own_stream && s->stream) (void)hipStreamDestroy(s->stream);
}

// Replaces the object's texture set with `pack` (the previous arrays are freed after the stream has drained).
int UploadPack(srt_surface* s, const srt::surface::TexturePack& pack) {
  SHIP_OK(hipSetDevice(s->device));
  uint32_t* texels = nullptr;
  uint4* info = nullptr;
  const size_t tb = pack.texels.size() * sizeof(uint32_t), ib = pack.info.size() * sizeof(uint32_t);
  SHIP_OK(hipMalloc(&texels, tb));
  if (hipError_t e = hipMalloc(&info, ib); e != hipSuccess) {
    (void)hipFree(texels);
    srt::SetError(std::string("srt_surface_upload_textures: hipMalloc: ") + hipGetErrorString(e));
    return SRT_ERR_HIP;
  }
  hipError_t e = hipMemcpyAsync(texels, pack.texels.data(), tb, hipMemcpyHostToDevice, s->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(info, pack.info.data(), ib, hipMemcpyHostToDevice, s->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(s->stream);  // the host arrays go out of scope; earlier launches are done
  if (e != hipSuccess) {
    (void)hipFree(texels);
    (void)hipFree(info);
    srt::SetError(std::string("srt_surface_upload_textures: ") + hipGetErrorString(e));
    return SRT_ERR_HIP;
  }
  if (s->d_texels) (void)hipFree(s->d_texels);
  if (s->d_tex_info) (void)hipFree(s->d_tex_info);
  s->d_texels = texels;
  s->d_tex_info = info;
  s->n_tex = pack.n;
  return SRT_OK;
}

int Upload(srt_surface* s, const srt::surface::Layout& lay) {
  SHIP_OK(hipSetDevice(s->device));
  if (!s->stream) {
    SHIP_OK(hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking));
    s->own_stream = true;
  }
  const size_t fb = lay.frames.size() * sizeof(float), tb = lay.tris.size() * sizeof(float4),
               mb = lay.mats.size() * sizeof(float4);
  SHIP_OK(hipMalloc(&s->d_frames, fb));
  SHIP_OK(hipMalloc(&s->d_tris, tb));
  SHIP_OK(hipMalloc(&s->d_mats, mb));
  SHIP_OK(hipMemcpyAsync(s->d_frames, lay.frames.data(), fb, hipMemcpyHostToDevice, s->stream));
  SHIP_OK(hipMemcpyAsync(s->d_tris, lay.tris.data(), tb, hipMemcpyHostToDevice, s->stream));
  SHIP_OK(hipMemcpyAsync(s->d_mats, lay.mats.data(), mb, hipMemcpyHostToDevice, s->stream));
  srt::surface::TexturePack none;
  std::string err;
  if (int rc = srt::surface::PackTextures(nullptr, 0, &none, &err)) return rc;
  return UploadPack(s, none);  // no texture yet: every handle is unknown (also waits for the copies above)
}

}  // namespace

extern "C" {

int srt_surface_abi_version(void) { return SRT_SURFACE_ABI_VERSION; }

int srt_surface_create(int device, void* stream, const srt_bvh_record* bvhs, uint32_t n_bvhs, const srt_material_obj* mats,
                       const float* tex_albedo, uint32_t n_mats, const srt_triangle* tris, uint32_t n_tris,
                       const srt_vertex* verts, uint32_t n_verts, srt_surface** out) {
  if (!out) return SRT_ERR_INVALID;
  *out = nullptr;
  // host-side validation and packing first: a bad scene never reaches the device
  srt::surface::Layout lay;
  std::string err;
  if (int rc = srt::surface::BuildLayout(bvhs, n_bvhs, mats, tex_albedo, n_mats, tris, n_tris, verts, n_verts, &lay, &err)) {
    srt::SetError(err);
    return rc;
  }
  srt_surface* s = new srt_surface();
  s->device = device;
  s->stream = static_cast<hipStream_t>(stream);
  s->n_bvhs = s->bvh_count = n_bvhs;
  s->n_tris = n_tris;
  if (int rc = Upload(s, lay)) {
    FreeAll(s);
    delete s;
    return rc;
  }
  *out = s;
  return SRT_OK;
}

int srt_surface_create_obj(int device, void* stream, const srt_scene* scene, srt_surface** out) {
  if (!scene || !out) return SRT_ERR_INVALID;
  *out = nullptr;
  uint32_t sz[5] = {0, 0, 0, 0, 0};
  if (int rc = srt_scene_sizes(scene, sz)) return rc;
  std::vector<srt_bvh_record> bvhs(sz[0]);
  std::vector<srt_bvh_node> nodes(sz[1]);
  std::vector<srt_material_obj> mats(sz[2]);
  std::vector<float> alb(3 * (size_t)sz[2]);
  std::vector<srt_triangle> tris(sz[3]);
  std::vector<srt_vertex> verts(sz[4]);
  if (int rc = srt_scene_copy(scene, bvhs.data(), nodes.data(), mats.data(), alb.data(), tris.data(), verts.data()))
    return rc;
  uint32_t n_tex = 0;
  int sample = 0;
  if (int rc = srt_scene_texture_count(scene, &n_tex, &sample)) return rc;
  std::vector<srt_texture> tx(sample ? n_tex : 0);
  for (uint32_t i = 0; i < (uint32_t)tx.size(); ++i)
    if (int rc = srt_scene_texture(scene, i, &tx[i])) return rc;
  srt::surface::TexturePack pack;
  if (sample) {  // validated before the object exists
    std::string err;
    if (int rc = srt::surface::PackTextures(tx.data(), (uint32_t)tx.size(), &pack, &err)) {
      srt::SetError(err);
      return rc;
    }
  }
  srt_surface* s = nullptr;
  if (int rc = srt_surface_create(device, stream, bvhs.data(), sz[0], mats.data(), sample ? nullptr : alb.data(), sz[2],
                                  tris.data(), sz[3], verts.data(), sz[4], &s))
    return rc;
  if (sample) {
    if (int rc = UploadPack(s, pack)) {
      srt_surface_destroy(s);
      return rc;
    }
  }
  *out = s;
  return SRT_OK;
}

int srt_surface_upload_textures(srt_surface* s, const srt_texture* textures, uint32_t n) {
  srt::surface::TexturePack pack;
  std::string err;
  if (int rc = srt::surface::PackTextures(textures, n, &pack, &err)) {  // before the object is looked at
    srt::SetError(err);
    return rc;
  }
  if (!s) return SRT_ERR_INVALID;
  return UploadPack(s, pack);
}

int srt_surface_update_model_matrix(srt_surface* s, uint32_t index, const float frame[16]) {
  if (!s || !frame) return SRT_ERR_INVALID;
  if (index >= s->n_bvhs) {
    srt::SetError("UpdateModelMatrix: index out of range");
    return SRT_ERR_INVALID;
  }
  SHIP_OK(hipSetDevice(s->device));
  // ordered with the launches on the stream; the 64 B leave `frame` before the call returns
  SHIP_OK(hipMemcpyAsync(s->d_frames + 16 * (size_t)index, frame, 16 * sizeof(float), hipMemcpyHostToDevice, s->stream));
  return SRT_OK;
}

int srt_surface_set_bvh_count(srt_surface* s, uint32_t bvh_count) {
  if (!s) return SRT_ERR_INVALID;
  s->bvh_count = bvh_count;
  return SRT_OK;
}

int srt_surface_destroy(srt_surface* s) {
  if (!s) return SRT_ERR_INVALID;
  (void)hipSetDevice(s->device);
  if (s->stream) (void)hipStreamSynchronize(s->stream);
  FreeAll(s);
  delete s;
  return SRT_OK;
}

void* srt_surface_stream(srt_surface* s) { return s ? s->stream : nullptr; }

int srt_surface_get_int(srt_surface* s, const char* name, int* v) {
  if (!s || !name || !v) return SRT_ERR_INVALID;
  const std::string n(name);
  if (n == "launch.blocks") *v = s->last_blocks;
  else if (n == "launch.block") *v = kBlock;
  else if (n == "textures") *v = (int)std::min<uint32_t>(s->n_tex, 0x7FFFFFFFu);
  else if (n == "bvh_count") *v = (int)s->bvh_count;
  else return SRT_ERR_NOT_FOUND;
  return SRT_OK;
}

int srt_surface_shade(srt_surface* s, const srt_ray* rays_dev, const srt_hit* hits_dev, uint32_t n,
                      srt_surface_attr* attrs_dev) {
  if (!s || (n && (!rays_dev || !hits_dev || !attrs_dev))) return SRT_ERR_INVALID;
  if (n == 0) return SRT_OK;
  if (((uintptr_t)rays_dev & 15u) || ((uintptr_t)hits_dev & 15u) || ((uintptr_t)attrs_dev & 15u)) {
    srt::SetError("srt_surface_shade: rays, hits and attrs must be 16-byte aligned");
    return SRT_ERR_INVALID;
  }
  SHIP_OK(hipSetDevice(s->device));
  SParams sp;
  std::memset(&sp, 0, sizeof sp);
  sp.frames = reinterpret_cast<const float4*>(s->d_frames);
  sp.tris = s->d_tris;
  sp.mats = s->d_mats;
  sp.texels = s->d_texels;
  sp.tex_info = s->d_tex_info;
  sp.rays = reinterpret_cast<const float4*>(rays_dev);
  sp.hits = reinterpret_cast<const uint4*>(hits_dev);
  sp.out = reinterpret_cast<float4*>(attrs_dev);
  sp.n = n;
  sp.n_bvhs = s->n_bvhs;
  sp.bvh_count = s->bvh_count;
  sp.n_tris = s->n_tris;
  sp.n_tex = s->n_tex;
  const unsigned blocks = (unsigned)(((uint64_t)n + kBlock - 1) / kBlock);
  hipLaunchKernelGGL(srt::surface::surface_shade_kernel, dim3(blocks), dim3(kBlock), 0, s->stream, sp);
  SHIP_OK(hipGetLastError());
  s->last_blocks = (int)blocks;
  return SRT_OK;
}

}  // extern "C"
