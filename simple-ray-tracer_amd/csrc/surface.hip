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
#include "../../include/srt_surface_refit.h"
#include "stage.hpp"
#include "surface.hpp"
#include "surface_host.hpp"

using srt::stage::Aligned;
using srt::stage::DevPtr;

struct srt_surface : srt::stage::Stage {
  DevPtr<float> d_frames;
  DevPtr<float4> d_tris, d_mats;
  DevPtr<uint32_t> d_texels;
  DevPtr<uint4> d_tex_info;
  uint32_t n_bvhs = 0, bvh_count = 0, n_tris = 0, n_tex = 0;
  int last_blocks = 0;
  DevPtr<uint4> d_triples;  // the triangles' vertex indices: only with SRT_SURFACE_REFIT (include/srt_surface_refit.h)
  bool refit = false;
  uint32_t n_verts = 0, refit_count = 0;
};

namespace {

using srt::surface::kBlock;
using srt::surface::SParams;

// Replaces the object's texture set with `pack` (the previous arrays are freed after the stream has drained).
int UploadPack(srt_surface* s, const srt::surface::TexturePack& pack) {
  STAGE_HIP_OK(hipSetDevice(s->device));
  DevPtr<uint32_t> texels;  // both, or (freed as they go out of scope) neither
  DevPtr<uint4> info;
  const size_t tb = pack.texels.size() * sizeof(uint32_t), ib = pack.info.size() * sizeof(uint32_t);
  STAGE_HIP_OK(texels.Alloc(tb));
  STAGE_HIP_OK(info.Alloc(ib));
  STAGE_HIP_OK(hipMemcpyAsync(texels, pack.texels.data(), tb, hipMemcpyHostToDevice, s->stream));
  STAGE_HIP_OK(hipMemcpyAsync(info, pack.info.data(), ib, hipMemcpyHostToDevice, s->stream));
  STAGE_HIP_OK(hipStreamSynchronize(s->stream));  // the host arrays go out of scope; earlier launches are done
  s->d_texels = std::move(texels);
  s->d_tex_info = std::move(info);
  s->n_tex = pack.n;
  return SRT_OK;
}

int Upload(srt_surface* s, const srt::surface::Layout& lay) {
  const size_t fb = lay.frames.size() * sizeof(float), tb = lay.tris.size() * sizeof(float4),
               mb = lay.mats.size() * sizeof(float4);
  STAGE_HIP_OK(s->d_frames.Alloc(fb));
  STAGE_HIP_OK(s->d_tris.Alloc(tb));
  STAGE_HIP_OK(s->d_mats.Alloc(mb));
  STAGE_HIP_OK(hipMemcpyAsync(s->d_frames, lay.frames.data(), fb, hipMemcpyHostToDevice, s->stream));
  STAGE_HIP_OK(hipMemcpyAsync(s->d_tris, lay.tris.data(), tb, hipMemcpyHostToDevice, s->stream));
  STAGE_HIP_OK(hipMemcpyAsync(s->d_mats, lay.mats.data(), mb, hipMemcpyHostToDevice, s->stream));
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
  return srt_surface_create_ex(device, stream, bvhs, n_bvhs, mats, tex_albedo, n_mats, tris, n_tris, verts, n_verts, 0u, out);
}

int srt_surface_create_ex(int device, void* stream, const srt_bvh_record* bvhs, uint32_t n_bvhs, const srt_material_obj* mats,
                          const float* tex_albedo, uint32_t n_mats, const srt_triangle* tris, uint32_t n_tris,
                          const srt_vertex* verts, uint32_t n_verts, uint32_t flags, srt_surface** out) {
  if (!out) return SRT_ERR_INVALID;
  *out = nullptr;
  if (flags & ~SRT_SURFACE_REFIT) {
    srt::SetError("srt_surface_create_ex: unknown flag");
    return SRT_ERR_INVALID;
  }
  // host-side validation and packing first: a bad scene never reaches the device
  srt::surface::Layout lay;
  std::string err;
  if (int rc = srt::surface::BuildLayout(bvhs, n_bvhs, mats, tex_albedo, n_mats, tris, n_tris, verts, n_verts, &lay, &err)) {
    srt::SetError(err);
    return rc;
  }
  srt::stage::Owned<srt_surface> s(new srt_surface());
  s->n_bvhs = s->bvh_count = n_bvhs;
  s->n_tris = n_tris;
  if (int rc = s->Acquire(device, stream)) return rc;
  if ((flags & SRT_SURFACE_REFIT) && n_tris) {  // ahead of Upload, whose wait for the stream covers this copy too
    static_assert(sizeof(srt_triangle) == sizeof(uint4), "the index triples are uploaded as they are");
    const size_t ib = (size_t)n_tris * sizeof(uint4);
    STAGE_HIP_OK(s->d_triples.Alloc(ib));
    STAGE_HIP_OK(hipMemcpyAsync(s->d_triples, tris, ib, hipMemcpyHostToDevice, s->stream));
  }
  if (int rc = Upload(s.get(), lay)) return rc;
  s->refit = (flags & SRT_SURFACE_REFIT) != 0;
  s->n_verts = n_verts;
  *out = s.release();
  return SRT_OK;
}

int srt_surface_create_obj(int device, void* stream, const srt_scene* scene, srt_surface** out) {
  return srt_surface_create_obj_ex(device, stream, scene, 0u, out);
}

int srt_surface_create_obj_ex(int device, void* stream, const srt_scene* scene, uint32_t flags, srt_surface** out) {
  if (!scene || !out) return SRT_ERR_INVALID;
  *out = nullptr;
  srt::stage::SceneArrays a;
  if (int rc = srt::stage::CopyScene(scene, &a)) return rc;
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
  srt_surface* created = nullptr;
  if (int rc = srt_surface_create_ex(device, stream, a.bvhs.data(), (uint32_t)a.bvhs.size(), a.mats.data(),
                                     sample ? nullptr : a.tex_albedo.data(), (uint32_t)a.mats.size(), a.tris.data(),
                                     (uint32_t)a.tris.size(), a.verts.data(), (uint32_t)a.verts.size(), flags, &created))
    return rc;
  srt::stage::Owned<srt_surface> s(created);
  if (sample) {
    if (int rc = UploadPack(s.get(), pack)) return rc;
  }
  *out = s.release();
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
  STAGE_HIP_OK(hipSetDevice(s->device));
  // ordered with the launches on the stream; the 64 B leave `frame` before the call returns
  STAGE_HIP_OK(hipMemcpyAsync(s->d_frames + 16 * (size_t)index, frame, 16 * sizeof(float), hipMemcpyHostToDevice, s->stream));
  return SRT_OK;
}

int srt_surface_set_bvh_count(srt_surface* s, uint32_t bvh_count) {
  if (!s) return SRT_ERR_INVALID;
  s->bvh_count = bvh_count;
  return SRT_OK;
}

int srt_surface_destroy(srt_surface* s) {
  if (!s) return SRT_ERR_INVALID;
  srt::stage::Destroy()(s);
  return SRT_OK;
}

void* srt_surface_stream(srt_surface* s) { return srt::stage::StreamOf(s); }

int srt_surface_get_int(srt_surface* s, const char* name, int* v) {
  if (!s || !name || !v) return SRT_ERR_INVALID;
  const std::string n(name);
  if (n == "launch.blocks") *v = s->last_blocks;
  else if (n == "launch.block") *v = kBlock;
  else if (n == "textures") *v = srt::stage::SaturateInt(s->n_tex);
  else if (n == "bvh_count") *v = (int)s->bvh_count;
  else if (n == "refit") *v = s->refit ? 1 : 0;
  else if (n == "refit.bytes") *v = srt::stage::SaturateInt(s->refit ? (size_t)s->n_tris * sizeof(uint4) : 0);
  else if (n == "refit.count") *v = (int)s->refit_count;
  else return SRT_ERR_NOT_FOUND;
  return SRT_OK;
}

int srt_surface_refit_abi_version(void) { return SRT_SURFACE_REFIT_ABI_VERSION; }

int srt_surface_refit(srt_surface* s, const srt_vertex* verts_dev, uint32_t n_verts) {
  if (!s) return SRT_ERR_INVALID;
  if (!s->refit) {
    srt::SetError("srt_surface_refit: the object was created without SRT_SURFACE_REFIT");
    return SRT_ERR_INVALID;
  }
  if (!verts_dev || !Aligned(verts_dev, 16)) {
    srt::SetError("srt_surface_refit: verts_dev must be a 16-byte aligned device pointer");
    return SRT_ERR_INVALID;
  }
  if (n_verts != s->n_verts) {
    srt::SetError("srt_surface_refit: n_verts differs from the count at creation");
    return SRT_ERR_INVALID;
  }
  STAGE_HIP_OK(hipSetDevice(s->device));
  if (s->n_tris) {
    const unsigned blocks = (unsigned)(((uint64_t)s->n_tris + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(srt::surface::surface_refit_kernel, dim3(blocks), dim3(kBlock), 0, s->stream, (float4*)s->d_tris,
                       (const uint4*)s->d_triples, reinterpret_cast<const float4*>(verts_dev), s->n_tris, n_verts);
    STAGE_HIP_OK(hipGetLastError());
  }
  ++s->refit_count;
  return SRT_OK;
}

int srt_surface_shade(srt_surface* s, const srt_ray* rays_dev, const srt_hit* hits_dev, uint32_t n,
                      srt_surface_attr* attrs_dev) {
  if (!s || (n && (!rays_dev || !hits_dev || !attrs_dev))) return SRT_ERR_INVALID;
  if (n == 0) return SRT_OK;
  if (!Aligned(rays_dev, 16) || !Aligned(hits_dev, 16) || !Aligned(attrs_dev, 16)) {
    srt::SetError("srt_surface_shade: rays, hits and attrs must be 16-byte aligned");
    return SRT_ERR_INVALID;
  }
  STAGE_HIP_OK(hipSetDevice(s->device));
  SParams sp;
  std::memset(&sp, 0, sizeof sp);
  sp.frames = reinterpret_cast<const float4*>(s->d_frames.get());
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
  STAGE_HIP_OK(hipGetLastError());
  s->last_blocks = (int)blocks;
  return SRT_OK;
}

}  // extern "C"
