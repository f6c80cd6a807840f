// temporal.hip -- the temporal reprojection of include/srt_temporal.h, include/srt_temporal_motion.h and
// include/srt_temporal_deform.h: the object, its ping-pong history, the poses' device arrays, the attached mesh and
// the launches of temporal.hpp's kernels.  A translation unit of its own, as query.hip and denoise.hip are:
// pathtrace.hip and its headers (the device code srt_code_hash identifies) are only read.
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>

#include "../../include/srt_temporal.h"
#include "../../include/srt_temporal_deform.h"
#include "../../include/srt_temporal_motion.h"
#include "../../include/srt_variance.h"
#include "denoise_host.hpp"
#include "stage.hpp"
#include "temporal.hpp"
#include "temporal_host.hpp"

using srt::stage::Aligned;
using srt::stage::DevPtr;

struct srt_temporal : srt::stage::Stage {
  int width = 0, height = 0;
  srt::temporal::Sizes sizes;
  DevPtr<float4> d_color[2];  // rgb | N
  DevPtr<float4> d_guide[2];  // normal | t
  DevPtr<uint32_t> d_id[2];   // BVH record, all ones for a miss
  srt_temporal_params params;
  srt::temporal::History hist;
  srt::temporal::Poses poses;
  DevPtr<uint4> d_motion;         // one MotionRecord per BVH record; grown by srt_temporal_set_models only
  uint32_t motion_capacity = 0;   // records
  DevPtr<float2> d_moments[2];    // m1 | m2 (include/srt_variance.h); allocated by srt_temporal_enable_moments
  srt::temporal::Moments moments;
  srt::temporal::Mesh mesh;         // include/srt_temporal_deform.h
  DevPtr<uint4> d_mesh_tris;        // the triangles' vertex indices; allocated by srt_temporal_set_mesh only
  DevPtr<float4> d_vprev;           // V': the positions the previous accumulate read
  DevPtr<uint4> d_deform;           // one DeformRecord per BVH record while a mesh is attached
  uint32_t deform_capacity = 0;     // records
  int last_launches = 0;
  int last_deform = 0;
};

namespace {

int Allocate(srt_temporal* tp) {
  STAGE_HIP_OK(srt::stage::AllocPair(tp->d_color, tp->sizes.color_bytes));
  STAGE_HIP_OK(srt::stage::AllocPair(tp->d_guide, tp->sizes.guide_bytes));
  STAGE_HIP_OK(srt::stage::AllocPair(tp->d_id, tp->sizes.id_bytes));
  return SRT_OK;
}

}  // namespace

extern "C" {

int srt_temporal_abi_version(void) { return SRT_TEMPORAL_ABI_VERSION; }

int srt_temporal_create(int device, void* stream, int width, int height, srt_temporal** out) {
  if (!out) return SRT_ERR_INVALID;
  *out = nullptr;
  srt::temporal::Sizes sizes;
  if (int rc = srt::temporal::PlanBuffers(width, height, &sizes)) {  // before any device is touched
    srt::SetError(rc == SRT_ERR_LIMIT ? "srt_temporal_create: image past 65535 in a dimension or 2^28 pixels"
                                      : "srt_temporal_create: width and height must be at least 1");
    return rc;
  }
  srt::stage::Owned<srt_temporal> tp(new srt_temporal());
  tp->width = width;
  tp->height = height;
  tp->sizes = sizes;
  tp->params = srt::temporal::DefaultParams();
  if (int rc = tp->Acquire(device, stream)) return rc;
  if (int rc = Allocate(tp.get())) return rc;
  *out = tp.release();
  return SRT_OK;
}

int srt_temporal_destroy(srt_temporal* tp) {
  if (!tp) return SRT_ERR_INVALID;
  srt::stage::Destroy()(tp);
  return SRT_OK;
}

void* srt_temporal_stream(srt_temporal* tp) { return srt::stage::StreamOf(tp); }

int srt_temporal_get_int(srt_temporal* tp, const char* name, int* v) {
  if (!tp || !name || !v) return SRT_ERR_INVALID;
  const std::string n(name);
  if (n == "width") *v = tp->width;
  else if (n == "height") *v = tp->height;
  else if (n == "max_history") *v = (int)tp->params.max_history;
  else if (n == "history") *v = tp->hist.valid ? 1 : 0;
  else if (n == "frames") *v = (int)tp->hist.frames;
  else if (n == "scratch.bytes") *v = srt::stage::SaturateInt(tp->sizes.scratch_bytes);
  else if (n == "launches") *v = tp->last_launches;
  else if (n == "models") *v = (int)tp->poses.cur.size();
  else if (n == "models.bytes") *v = (int)(tp->motion_capacity * sizeof(srt::temporal::MotionRecord));
  else if (n == "mesh.tris") *v = (int)tp->mesh.n_tris;
  else if (n == "mesh.verts") *v = (int)tp->mesh.n_verts;
  else if (n == "mesh.bytes")
    *v = srt::stage::SaturateInt(srt::temporal::MeshBytes(tp->mesh) + (size_t)tp->deform_capacity * sizeof(srt::temporal::DeformRecord));
  else if (n == "deform") *v = tp->last_deform;
  else if (n == "moments.bytes") *v = srt::stage::SaturateInt(tp->moments.enabled ? 2 * srt::temporal::MomentBytes(tp->sizes) : 0);
  else return SRT_ERR_NOT_FOUND;
  return SRT_OK;
}

int srt_temporal_get_params(srt_temporal* tp, srt_temporal_params* p) {
  if (!tp || !p) return SRT_ERR_INVALID;
  *p = tp->params;
  return SRT_OK;
}

int srt_temporal_set_params(srt_temporal* tp, const srt_temporal_params* p) {
  if (!tp) return SRT_ERR_INVALID;
  if (int rc = srt::temporal::ValidateParams(p)) {
    srt::SetError("srt_temporal_set_params: max_history 1..65535, depth_tol finite and > 0, normal_min in [-1, 1]");
    return rc;
  }
  tp->params = *p;
  return SRT_OK;
}

int srt_temporal_reset(srt_temporal* tp) {
  if (!tp) return SRT_ERR_INVALID;
  srt::temporal::Reset(&tp->hist);
  srt::temporal::ResetPoses(&tp->poses);
  srt::temporal::ResetMoments(&tp->moments);
  srt::temporal::ResetMesh(&tp->mesh);
  return SRT_OK;
}

}  // extern "C"

namespace {

// Both accumulate functions: out_moments_dev is NULL for srt_temporal_accumulate.
int Accumulate(srt_temporal* tp, const void* accum_rgba32f_dev, int frames, const srt_hit* guide_dev,
               const srt_temporal_camera* cam, void* out_rgba32f_dev, void* out_moments_dev) {
  if (!tp || !accum_rgba32f_dev || !guide_dev || !cam || !out_rgba32f_dev || frames < 1) return SRT_ERR_INVALID;
  if (!Aligned(accum_rgba32f_dev, 16) || !Aligned(guide_dev, 16) || !Aligned(out_rgba32f_dev, 16)) {
    srt::SetError("srt_temporal_accumulate: accum, guide and out must be 16-byte aligned");
    return SRT_ERR_INVALID;
  }
  if (out_rgba32f_dev == accum_rgba32f_dev || out_rgba32f_dev == (const void*)guide_dev) {
    srt::SetError("srt_temporal_accumulate: out may not alias the inputs");
    return SRT_ERR_INVALID;
  }
  STAGE_HIP_OK(hipSetDevice(tp->device));
  using namespace srt::temporal;
  TParams kp;
  std::memset(&kp, 0, sizeof kp);
  const int rd = tp->hist.read, wr = WriteIndex(tp->hist);
  kp.accum = static_cast<const float4*>(accum_rgba32f_dev);
  kp.hits = reinterpret_cast<const uint4*>(guide_dev);
  kp.pcol = tp->d_color[rd];
  kp.pgd = tp->d_guide[rd];
  kp.pid = tp->d_id[rd];
  kp.ncol = tp->d_color[wr];
  kp.ngd = tp->d_guide[wr];
  kp.nid = tp->d_id[wr];
  kp.out = static_cast<float4*>(out_rgba32f_dev);
  kp.W = tp->width;
  kp.H = tp->height;
  kp.has_prev = tp->hist.valid ? 1 : 0;
  kp.frames = (float)frames;
  kp.max_history = (float)tp->params.max_history;
  kp.depth_tol = tp->params.depth_tol;
  kp.normal_min = tp->params.normal_min;
  srt::denoise::Basis b;
  srt::denoise::PrimaryBasis(cam->origin, cam->front, cam->right, cam->up, tp->width, tp->height, &b);
  std::memcpy(kp.o, b.o, sizeof kp.o);
  std::memcpy(kp.p00, b.p00, sizeof kp.p00);
  std::memcpy(kp.du, b.du, sizeof kp.du);
  std::memcpy(kp.dv, b.dv, sizeof kp.dv);
  const srt_temporal_camera& pc = tp->hist.prev;
  std::memcpy(kp.po, pc.origin, sizeof kp.po);
  std::memcpy(kp.pf, pc.front, sizeof kp.pf);
  std::memcpy(kp.pr, pc.right, sizeof kp.pr);
  std::memcpy(kp.pu, pc.up, sizeof kp.pu);
  MParams mp;
  std::memset(&mp, 0, sizeof mp);
  if (out_moments_dev) {
    mp.pm = tp->d_moments[rd];
    mp.nm = tp->d_moments[wr];
    mp.out = static_cast<float4*>(out_moments_dev);
    mp.has_prev = MomentsHavePrev(tp->moments, tp->hist);
  }
  const uint32_t n = (uint32_t)tp->poses.cur.size();  // <= motion_capacity: srt_temporal_set_models grew the array
  const dim3 grid(tp->sizes.grid_x, tp->sizes.grid_y);
  const bool deform = DeformRuns(tp->mesh);
  if (deform) {
    // srt_temporal_set_mesh and srt_temporal_set_models grew d_deform to n records; the chunks travel as the
    // motion records do.
    MotionChunk chunk;
    DeformChunk dchunk;
    for (uint32_t first = 0; first < n; first += kUploadChunk) {
      const uint32_t count = FillChunk(tp->poses, first, &chunk);
      hipLaunchKernelGGL(temporal_motion_upload_kernel, dim3(1), dim3(kUploadLanes), 0, tp->stream, chunk, tp->d_motion, first, count);
      FillDeformChunk(tp->poses, first, &dchunk);
      hipLaunchKernelGGL(temporal_deform_upload_kernel, dim3(1), dim3(kDeformUploadLanes), 0, tp->stream, dchunk, tp->d_deform, first,
                         count);
    }
    DParams dp;
    std::memset(&dp, 0, sizeof dp);
    dp.tris = tp->d_mesh_tris;
    dp.verts = static_cast<const float4*>(tp->mesh.verts);
    dp.vprev = tp->d_vprev;
    dp.recs = tp->d_deform;
    dp.n_tris = tp->mesh.n_tris;
    dp.n_verts = tp->mesh.n_verts;
    dp.has_vprev = DeformHasPrev(tp->mesh, tp->hist);
    if (out_moments_dev)
      hipLaunchKernelGGL(temporal_accumulate_deform_moments_kernel, grid, dim3(kBlock), 0, tp->stream, kp, mp, dp,
                         (const uint4*)tp->d_motion, n);
    else
      hipLaunchKernelGGL(temporal_accumulate_deform_kernel, grid, dim3(kBlock), 0, tp->stream, kp, dp, (const uint4*)tp->d_motion, n);
    // V becomes V' behind the kernel that read both
    hipLaunchKernelGGL(temporal_copy_positions_kernel, dim3((dp.n_verts + kBlock - 1) / kBlock), dim3(kBlock), 0, tp->stream, dp.verts,
                       (float4*)tp->d_vprev, dp.n_verts);
  } else if (n == 0) {
    if (out_moments_dev)
      hipLaunchKernelGGL(temporal_accumulate_moments_kernel, grid, dim3(kBlock), 0, tp->stream, kp, mp);
    else
      hipLaunchKernelGGL(temporal_accumulate_kernel, grid, dim3(kBlock), 0, tp->stream, kp);
  } else {
    // The records travel in kernel arguments, which the launch copies before it returns; stream order puts them
    // behind the previous frame's kernel, so one device array serves.
    MotionChunk chunk;
    for (uint32_t first = 0; first < n; first += kUploadChunk) {
      const uint32_t count = FillChunk(tp->poses, first, &chunk);
      hipLaunchKernelGGL(temporal_motion_upload_kernel, dim3(1), dim3(kUploadLanes), 0, tp->stream, chunk, tp->d_motion, first, count);
    }
    if (out_moments_dev)
      hipLaunchKernelGGL(temporal_accumulate_motion_moments_kernel, grid, dim3(kBlock), 0, tp->stream, kp, mp,
                         (const uint4*)tp->d_motion, n);
    else
      hipLaunchKernelGGL(temporal_accumulate_motion_kernel, grid, dim3(kBlock), 0, tp->stream, kp, (const uint4*)tp->d_motion, n);
  }
  STAGE_HIP_OK(hipGetLastError());
  Advance(&tp->hist, *cam);
  AdvancePoses(&tp->poses);
  AdvanceMoments(&tp->moments, out_moments_dev != nullptr);
  AdvanceMesh(&tp->mesh);
  tp->last_launches = Launches(n, deform);
  tp->last_deform = deform ? 1 : 0;
  return SRT_OK;
}

}  // namespace

extern "C" {

int srt_temporal_accumulate(srt_temporal* tp, const void* accum_rgba32f_dev, int frames, const srt_hit* guide_dev,
                            const srt_temporal_camera* cam, void* out_rgba32f_dev) {
  return Accumulate(tp, accum_rgba32f_dev, frames, guide_dev, cam, out_rgba32f_dev, nullptr);
}

int srt_temporal_enable_moments(srt_temporal* tp) {
  if (!tp) return SRT_ERR_INVALID;
  if (tp->moments.enabled) return SRT_OK;
  STAGE_HIP_OK(hipSetDevice(tp->device));
  STAGE_HIP_OK(srt::stage::AllocPair(tp->d_moments, srt::temporal::MomentBytes(tp->sizes)));
  srt::temporal::EnableMoments(&tp->moments);
  return SRT_OK;
}

int srt_temporal_accumulate_moments(srt_temporal* tp, const void* accum_rgba32f_dev, int frames, const srt_hit* guide_dev,
                                    const srt_temporal_camera* cam, void* out_rgba32f_dev, void* out_moments_dev) {
  if (!tp || !out_moments_dev) return SRT_ERR_INVALID;
  if (!tp->moments.enabled) {
    srt::SetError("srt_temporal_accumulate_moments: call srt_temporal_enable_moments first");
    return SRT_ERR_INVALID;
  }
  if (!Aligned(out_moments_dev, 16) || out_moments_dev == accum_rgba32f_dev || out_moments_dev == (const void*)guide_dev ||
      out_moments_dev == out_rgba32f_dev) {
    srt::SetError("srt_temporal_accumulate_moments: out_moments must be 16-byte aligned and alias no other pointer");
    return SRT_ERR_INVALID;
  }
  return Accumulate(tp, accum_rgba32f_dev, frames, guide_dev, cam, out_rgba32f_dev, out_moments_dev);
}

int srt_temporal_motion_abi_version(void) { return SRT_TEMPORAL_MOTION_ABI_VERSION; }

}  // extern "C"

namespace {

// The deform records' array holds a record per pose while a mesh is attached; objects without a mesh have none.
int GrowDeform(srt_temporal* tp, uint32_t n) {
  if (tp->mesh.n_tris == 0 || n <= tp->deform_capacity) return SRT_OK;
  STAGE_HIP_OK(hipSetDevice(tp->device));
  DevPtr<uint4> grown;
  STAGE_HIP_OK(grown.Alloc((size_t)n * sizeof(srt::temporal::DeformRecord)));
  if (tp->d_deform) (void)hipStreamSynchronize(tp->stream);  // an enqueued frame may still read the old array
  tp->d_deform = std::move(grown);
  tp->deform_capacity = n;
  return SRT_OK;
}

}  // namespace

extern "C" {

int srt_temporal_set_models(srt_temporal* tp, const srt_temporal_model* models, uint32_t n) {
  if (int rc = srt::temporal::ValidateModels(models, n)) {  // before the object or any device is touched
    srt::SetError(rc == SRT_ERR_LIMIT ? "srt_temporal_set_models: more than 65535 records"
                                      : "srt_temporal_set_models: every entry finite and each bottom row (0, 0, 0, 1)");
    return rc;
  }
  if (!tp) {
    srt::SetError("srt_temporal_set_models: NULL object");
    return SRT_ERR_INVALID;
  }
  if (n > tp->motion_capacity) {
    STAGE_HIP_OK(hipSetDevice(tp->device));
    DevPtr<uint4> grown;
    STAGE_HIP_OK(grown.Alloc((size_t)n * sizeof(srt::temporal::MotionRecord)));
    if (tp->d_motion) (void)hipStreamSynchronize(tp->stream);  // an enqueued frame may still read the old array
    tp->d_motion = std::move(grown);
    tp->motion_capacity = n;
  }
  if (int rc = GrowDeform(tp, n)) return rc;
  return srt::temporal::SetModels(&tp->poses, models, n);
}

int srt_temporal_deform_abi_version(void) { return SRT_TEMPORAL_DEFORM_ABI_VERSION; }

int srt_temporal_set_mesh(srt_temporal* tp, const srt_triangle* tris, uint32_t n_tris, uint32_t n_verts) {
  static_assert(sizeof(srt_triangle) == sizeof(uint4), "the index triples are uploaded as they are");
  if (int rc = srt::temporal::ValidateMesh(tris, n_tris, n_verts)) {  // before the object or any device is touched
    srt::SetError(rc == SRT_ERR_LIMIT ? "srt_temporal_set_mesh: 2^28 triangles or vertices, or more"
                                      : "srt_temporal_set_mesh: NULL tris or n_verts == 0 with n_tris > 0");
    return rc;
  }
  if (!tp) {
    srt::SetError("srt_temporal_set_mesh: NULL object");
    return SRT_ERR_INVALID;
  }
  STAGE_HIP_OK(hipSetDevice(tp->device));
  if (n_tris == 0) {
    STAGE_HIP_OK(hipStreamSynchronize(tp->stream));  // an enqueued frame may still read the arrays
    tp->d_mesh_tris = DevPtr<uint4>();
    tp->d_vprev = DevPtr<float4>();
    tp->d_deform = DevPtr<uint4>();
    tp->deform_capacity = 0;
    return srt::temporal::AttachMesh(&tp->mesh, nullptr, 0, 0);
  }
  DevPtr<uint4> idx;  // all, or (freed as they go out of scope) none
  DevPtr<float4> vprev;
  const size_t tb = (size_t)n_tris * sizeof(uint4);
  STAGE_HIP_OK(idx.Alloc(tb));
  STAGE_HIP_OK(vprev.Alloc((size_t)n_verts * sizeof(float4)));
  STAGE_HIP_OK(hipMemcpyAsync(idx, tris, tb, hipMemcpyHostToDevice, tp->stream));
  STAGE_HIP_OK(hipStreamSynchronize(tp->stream));  // `tris` may go; an enqueued frame no longer reads the old arrays
  tp->d_mesh_tris = std::move(idx);
  tp->d_vprev = std::move(vprev);
  if (int rc = srt::temporal::AttachMesh(&tp->mesh, tris, n_tris, n_verts)) return rc;
  return GrowDeform(tp, (uint32_t)tp->poses.cur.size());
}

int srt_temporal_set_vertices(srt_temporal* tp, const srt_vertex* verts_dev, uint32_t n_verts) {
  if (!Aligned(verts_dev, 16)) {
    srt::SetError("srt_temporal_set_vertices: verts_dev must be 16-byte aligned");
    return SRT_ERR_INVALID;
  }
  if (!tp) {
    srt::SetError("srt_temporal_set_vertices: NULL object");
    return SRT_ERR_INVALID;
  }
  if (int rc = srt::temporal::SetVertices(&tp->mesh, verts_dev, n_verts)) {
    srt::SetError(tp->mesh.n_tris == 0 ? "srt_temporal_set_vertices: no mesh attached (srt_temporal_set_mesh)"
                                       : "srt_temporal_set_vertices: n_verts differs from the mesh's");
    return rc;
  }
  return SRT_OK;
}

int srt_temporal_model_from_frame(const float frame[16], srt_temporal_model* out) {
  if (int rc = srt::temporal::ModelFromFrame(frame, out)) {
    srt::SetError("srt_temporal_model_from_frame: a finite, affine, non-singular frame");
    return rc;
  }
  return SRT_OK;
}

}  // extern "C"
