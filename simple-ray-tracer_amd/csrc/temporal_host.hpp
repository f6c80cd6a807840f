// temporal_host.hpp -- host-only parts of the temporal reprojection (include/srt_temporal.h): parameter
// validation, buffer sizing, the launch grid and the ping-pong state of the history, and the pose bookkeeping
// of include/srt_temporal_motion.h and the mesh bookkeeping of include/srt_temporal_deform.h.  No device, no HIP
// header: tests/cpp/test_temporal_host.cpp, tests/cpp/test_temporal_motion_host.cpp and
// tests/cpp/test_temporal_deform_host.cpp link temporal_host.cpp alone.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/srt_temporal.h"
#include "../../include/srt_temporal_deform.h"
#include "../../include/srt_temporal_motion.h"

namespace srt {
namespace temporal {

constexpr int kBlock = 256;              // lanes per block
constexpr int kRowW = 64, kRowH = 4;     // pixels of a block: a wave is 64 contiguous pixels of one row
constexpr int kMaxDim = 65535;
constexpr uint64_t kMaxPixels = 1ull << 28;

srt_temporal_params DefaultParams();
// SRT_OK, or SRT_ERR_INVALID: NULL, max_history outside 1..65535, depth_tol not finite and > 0, normal_min not
// finite or outside [-1, 1].
int ValidateParams(const srt_temporal_params* p);

struct Sizes {
  uint64_t pixels = 0;
  size_t color_bytes = 0;    // one history colour buffer: float4 (rgb | N) per pixel
  size_t guide_bytes = 0;    // one packed guide: float4 (normal | t) per pixel
  size_t id_bytes = 0;       // one id array: the hit's BVH record, all ones for a miss
  size_t scratch_bytes = 0;  // two of each: the kernel reads arbitrary previous pixels while it writes
  unsigned grid_x = 0, grid_y = 0;
};
// SRT_OK; SRT_ERR_INVALID for a dimension < 1 or NULL `out`; SRT_ERR_LIMIT past kMaxDim or kMaxPixels.
int PlanBuffers(int width, int height, Sizes* out);

// The history's state: which of the two buffer sets holds the previous frame, whether it holds one at all, and
// the accumulate calls since the last reset.
struct History {
  int read = 0;        // the set the next call reads; it writes set `read ^ 1`
  bool valid = false;  // set `read` holds a previous frame (and `prev` its camera)
  uint32_t frames = 0;
  srt_temporal_camera prev = {};
};
void Reset(History* h);
inline int WriteIndex(const History& h) { return h.read ^ 1; }
// After a call was enqueued: the written set becomes the one to read, `cam` the previous camera.
void Advance(History* h, const srt_temporal_camera& cam);

// ---- moving models (include/srt_temporal_motion.h) ----

constexpr uint32_t kMaxModels = SRT_TEMPORAL_MAX_MODELS;
constexpr uint32_t kUploadChunk = SRT_TEMPORAL_MODELS_PER_LAUNCH;  // records one upload launch carries by value

// What the device sees per BVH record, 64 B: the rows of M_r as three 16-B words (row i = M(i,0..3)), then a
// word whose first component is 1 for a MOVING record and 0 for a STATIC one.
struct MotionRecord {
  float m[12];
  uint32_t moving;
  uint32_t pad[3];
};
static_assert(sizeof(MotionRecord) == 64, "one 64-B record");
struct MotionChunk {
  MotionRecord r[kUploadChunk];
};

// SRT_OK; SRT_ERR_INVALID for NULL with n > 0, an entry that is not finite or a bottom row that is not exactly
// (0, 0, 0, 1); SRT_ERR_LIMIT for n > kMaxModels.
int ValidateModels(const srt_temporal_model* models, uint32_t n);
int ModelFromFrame(const float frame[16], srt_temporal_model* out);

// P (the poses of the previous accumulated frame; empty when there is none) and Q (the current ones).
struct Poses {
  std::vector<srt_temporal_model> cur;   // Q
  std::vector<srt_temporal_model> prev;  // P
};
// ValidateModels, then Q = models (state unchanged on an error).
int SetModels(Poses* p, const srt_temporal_model* models, uint32_t n);
// M = a.model_to_world o b.world_to_model, rows of four, in the element order the header writes down.
void ComposeMotion(const srt_temporal_model& a, const srt_temporal_model& b, float m[12]);
// Record r of the frame about to be accumulated.  A STATIC record gets the identity, which the kernel does not
// apply.
MotionRecord MotionOf(const Poses& p, uint32_t r);
// Records [first, first + kUploadChunk) of Q, zero past its end; returns how many are real.
uint32_t FillChunk(const Poses& p, uint32_t first, MotionChunk* out);
inline uint32_t UploadLaunches(uint32_t n) { return (n + kUploadChunk - 1) / kUploadChunk; }
// After a call was enqueued: Q becomes P.  With the history's Reset: P is dropped, Q stays.
void AdvancePoses(Poses* p);
void ResetPoses(Poses* p);

// ---- deforming meshes (include/srt_temporal_deform.h) ----

constexpr uint32_t kMaxMesh = SRT_TEMPORAL_MAX_MESH;

// SRT_OK; SRT_ERR_LIMIT for a count >= kMaxMesh; SRT_ERR_INVALID for NULL `tris` or n_verts == 0 with n_tris > 0.
// The counts are checked before the array.
int ValidateMesh(const srt_triangle* tris, uint32_t n_tris, uint32_t n_verts);

// The attached mesh, V (the caller's device array; only its address is held here) and whether V' -- the object's
// copy of the positions the previous accumulate read -- holds any.
struct Mesh {
  uint32_t n_tris = 0, n_verts = 0;  // n_tris == 0: no mesh
  const void* verts = nullptr;       // V
  bool has_prev = false;             // V' is valid
};
// ValidateMesh, then the counts; V and V' are dropped.  n_tris == 0 detaches.
int AttachMesh(Mesh* m, const srt_triangle* tris, uint32_t n_tris, uint32_t n_verts);
// srt_temporal_set_vertices on an existing object: SRT_ERR_INVALID (state unchanged) for a pointer that is not
// 16-B aligned, no mesh, or n_verts != the mesh's.  NULL drops V and V'.
int SetVertices(Mesh* m, const void* verts_dev, uint32_t n_verts);
// Whether the accumulate about to be enqueued runs a deform instance, and whether that instance finds V'.
inline bool DeformRuns(const Mesh& m) { return m.n_tris > 0 && m.verts != nullptr; }
inline int DeformHasPrev(const Mesh& m, const History& h) { return DeformRuns(m) && m.has_prev && h.valid ? 1 : 0; }
// After a call was enqueued: a deform instance's copy made V' valid.  With the history's Reset: V' is dropped.
void AdvanceMesh(Mesh* m);
void ResetMesh(Mesh* m);
// Device bytes of the vertex indices and of V' (the deform records are counted by their capacity, next to them).
inline size_t MeshBytes(const Mesh& m) { return m.n_tris ? ((size_t)m.n_tris + (size_t)m.n_verts) * 16 : 0; }

// What a deform instance reads per BVH record next to its MotionRecord, 96 B: the rows of Q[r].world_to_model,
// then the rows of A (P[r].model_to_world when r < n_P, else Q[r].model_to_world), row i = M(i, 0..3).
struct DeformRecord {
  float w2m[12];
  float a[12];
};
static_assert(sizeof(DeformRecord) == 96, "six 16-B words");
struct DeformChunk {
  DeformRecord r[kUploadChunk];
};
DeformRecord DeformOf(const Poses& p, uint32_t r);
// Records [first, first + kUploadChunk) of Q, zero past its end; returns how many are real.
uint32_t FillDeformChunk(const Poses& p, uint32_t first, DeformChunk* out);
// Launches of one accumulate with n poses: the kernel and the motion uploads, and for a deform instance the
// deform records' uploads and the copy of V into V'.
inline int Launches(uint32_t n, bool deform) { return 1 + (int)UploadLaunches(n) + (deform ? (int)UploadLaunches(n) + 1 : 0); }

// ---- luminance moments (include/srt_variance.h) ----

// One moment array: float2 (m1 | m2) per pixel.  The object holds two, indexed as the colour history's sets are
// (History::read and WriteIndex), and they are no part of Sizes::scratch_bytes.
inline size_t MomentBytes(const Sizes& s) { return (size_t)s.pixels * 8; }
// Whether the arrays exist and whether set History::read holds the moments of the previous frame.
struct Moments {
  bool enabled = false;
  bool valid = false;
};
// srt_temporal_enable_moments: idempotent; a history that existed before has no moments.
void EnableMoments(Moments* m);
// 1 when the call about to be enqueued finds moments of the previous frame (and a colour history to go with them).
inline int MomentsHavePrev(const Moments& m, const History& h) { return m.enabled && m.valid && h.valid ? 1 : 0; }
// After a call was enqueued: `with_moments` tells which of the two accumulate functions it was.
void AdvanceMoments(Moments* m, bool with_moments);
void ResetMoments(Moments* m);

}  // namespace temporal
}  // namespace srt
