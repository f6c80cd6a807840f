// Stand-alone checks of the mesh bookkeeping of include/srt_temporal_deform.h (csrc/temporal_host.cpp, no HIP, no
// device): validation, which instance runs, the launch counts, V and V' over set_mesh / set_vertices / reset, and
// the deform records.  Built with -fsanitize=address,undefined by tests/test_temporal_deform_api.py and by
// `make SAN=1 test_temporal_deform_host`.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../simple-ray-tracer_amd/csrc/temporal_host.hpp"

using namespace srt::temporal;

#define CHECK(c)                                                      \
  do {                                                                \
    if (!(c)) {                                                       \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);      \
      std::exit(1);                                                   \
    }                                                                 \
  } while (0)

static srt_temporal_model Pose(float tx, float s) {
  srt_temporal_model m;
  std::memset(&m, 0, sizeof m);
  for (int k = 0; k < 3; ++k) {
    m.world_to_model[5 * k] = s;
    m.model_to_world[5 * k] = 1.0f / s;
  }
  m.world_to_model[15] = m.model_to_world[15] = 1.0f;
  m.world_to_model[12] = -tx * s;
  m.world_to_model[6] = 0.25f;  // (row 2, column 1): tells rows from columns
  m.model_to_world[12] = tx;
  return m;
}

int main() {
  std::vector<srt_triangle> tris(32);
  alignas(16) static float storage[64];
  const void* verts = storage;

  // validation: the counts, then the array
  CHECK(ValidateMesh(tris.data(), 32, 25) == SRT_OK);
  CHECK(ValidateMesh(nullptr, 0, 0) == SRT_OK && ValidateMesh(nullptr, 0, 7) == SRT_OK);
  CHECK(ValidateMesh(nullptr, 32, 25) == SRT_ERR_INVALID);
  CHECK(ValidateMesh(tris.data(), 32, 0) == SRT_ERR_INVALID);
  CHECK(ValidateMesh(tris.data(), 1u << 28, 25) == SRT_ERR_LIMIT && ValidateMesh(tris.data(), 32, 1u << 28) == SRT_ERR_LIMIT);
  CHECK(ValidateMesh(nullptr, 0xFFFFFFFFu, 0) == SRT_ERR_LIMIT);
  CHECK(ValidateMesh(tris.data(), (1u << 28) - 1, (1u << 28) - 1) == SRT_OK);

  Mesh m;
  History h;
  srt_temporal_camera cam = {};
  // an object never given a mesh: today's kernels and launch counts
  CHECK(!DeformRuns(m) && DeformHasPrev(m, h) == 0 && MeshBytes(m) == 0);
  CHECK(Launches(0, false) == 1 && Launches(1, false) == 2 && Launches(32, false) == 2 && Launches(33, false) == 3);
  CHECK(Launches(70, false) == 1 + (int)UploadLaunches(70));
  // set_vertices without a mesh, and a failed attach, change nothing
  CHECK(SetVertices(&m, verts, 25) == SRT_ERR_INVALID && m.verts == nullptr);
  CHECK(AttachMesh(&m, nullptr, 32, 25) == SRT_ERR_INVALID && m.n_tris == 0);
  CHECK(AttachMesh(&m, tris.data(), 1u << 28, 25) == SRT_ERR_LIMIT && m.n_tris == 0);
  CHECK(AttachMesh(nullptr, tris.data(), 32, 25) == SRT_ERR_INVALID);

  CHECK(AttachMesh(&m, tris.data(), 32, 25) == SRT_OK && m.n_tris == 32 && m.n_verts == 25);
  CHECK(MeshBytes(m) == 16 * (32 + 25));
  CHECK(!DeformRuns(m));  // a mesh without V: the instances of before
  CHECK(SetVertices(&m, verts, 24) == SRT_ERR_INVALID && SetVertices(&m, nullptr, 24) == SRT_ERR_INVALID && m.verts == nullptr);
  CHECK(SetVertices(&m, static_cast<const char*>(verts) + 4, 25) == SRT_ERR_INVALID && m.verts == nullptr);
  CHECK(SetVertices(&m, static_cast<const char*>(verts) + 8, 25) == SRT_ERR_INVALID);
  CHECK(SetVertices(&m, verts, 25) == SRT_OK && m.verts == verts);
  // frame 0: the deform instance runs (it makes V'), every pixel RIGID: no history, no V'
  CHECK(DeformRuns(m) && DeformHasPrev(m, h) == 0);
  CHECK(Launches(0, true) == 2 && Launches(1, true) == 4 && Launches(32, true) == 4 && Launches(33, true) == 6);
  Advance(&h, cam);
  AdvanceMesh(&m);
  CHECK(m.has_prev && DeformHasPrev(m, h) == 1);
  // reset: V' and the history go, V stays; one frame later both are back
  Reset(&h);
  ResetMesh(&m);
  CHECK(DeformRuns(m) && !m.has_prev && DeformHasPrev(m, h) == 0);
  Advance(&h, cam);
  AdvanceMesh(&m);
  CHECK(DeformHasPrev(m, h) == 1);
  // V' without a history is no V' (a reset of the history alone cannot happen through the C ABI; the rule holds anyway)
  Reset(&h);
  CHECK(DeformHasPrev(m, h) == 0);
  Advance(&h, cam);
  // set_vertices(NULL): RIGID, V' dropped, the instances of before; a frame accumulated meanwhile makes no V'
  CHECK(SetVertices(&m, nullptr, 25) == SRT_OK && !DeformRuns(m) && !m.has_prev);
  AdvanceMesh(&m);
  CHECK(!m.has_prev);
  CHECK(SetVertices(&m, verts, 25) == SRT_OK && DeformRuns(m) && DeformHasPrev(m, h) == 0);
  AdvanceMesh(&m);
  CHECK(DeformHasPrev(m, h) == 1);
  // a new mesh drops V and V'; n_tris == 0 detaches
  CHECK(AttachMesh(&m, tris.data(), 8, 9) == SRT_OK && m.n_tris == 8 && m.verts == nullptr && !m.has_prev);
  CHECK(SetVertices(&m, verts, 9) == SRT_OK);
  CHECK(AttachMesh(&m, nullptr, 0, 0) == SRT_OK && m.n_tris == 0 && m.n_verts == 0 && !DeformRuns(m) && MeshBytes(m) == 0);
  CHECK(SetVertices(&m, verts, 9) == SRT_ERR_INVALID);

  // the deform records: rows of Q.world_to_model, then rows of P.model_to_world, or Q's while P has no such record
  Poses p;
  const srt_temporal_model q0 = Pose(1.0f, 2.0f), q1 = Pose(-3.0f, 0.5f), p0 = Pose(0.5f, 2.0f);
  const srt_temporal_model cur[2] = {q0, q1};
  CHECK(SetModels(&p, cur, 2) == SRT_OK);
  DeformRecord r = DeformOf(p, 0);  // n_P == 0: A = Q.model_to_world
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 4; ++j) {
      CHECK(r.w2m[4 * i + j] == q0.world_to_model[4 * j + i]);
      CHECK(r.a[4 * i + j] == q0.model_to_world[4 * j + i]);
    }
  CHECK(r.w2m[4 * 2 + 1] == 0.25f && r.w2m[4 * 1 + 2] == 0.0f);
  p.prev.assign(1, p0);  // n_P == 1: record 0 takes P's, record 1 (n_P <= r < n_Q) Q's
  r = DeformOf(p, 0);
  CHECK(r.a[3] == 0.5f && r.w2m[3] == q0.world_to_model[12]);
  r = DeformOf(p, 1);
  CHECK(r.a[3] == -3.0f && r.a[0] == 2.0f && r.w2m[0] == 0.5f);
  r = DeformOf(p, 2);  // past Q: zeros, never read
  for (int k = 0; k < 12; ++k) CHECK(r.w2m[k] == 0.0f && r.a[k] == 0.0f);
  DeformChunk chunk;
  CHECK(FillDeformChunk(p, 0, &chunk) == 2 && chunk.r[1].a[3] == -3.0f && chunk.r[2].a[0] == 0.0f);
  CHECK(FillDeformChunk(p, 32, &chunk) == 0);
  std::vector<srt_temporal_model> many(70, q1);
  CHECK(SetModels(&p, many.data(), 70) == SRT_OK);
  CHECK(FillDeformChunk(p, 0, &chunk) == 32 && FillDeformChunk(p, 64, &chunk) == 6 && chunk.r[5].a[3] == -3.0f && chunk.r[6].a[3] == 0.0f);
  CHECK(Launches(70, true) == 1 + 3 + 3 + 1);
  static_assert(sizeof(DeformChunk) == 32 * 96 && sizeof(DeformChunk) + 64 <= 4096, "a chunk fits the kernel arguments");

  std::printf("temporal deform host checks OK\n");
  return 0;
}
