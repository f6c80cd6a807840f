// temporal_host.cpp -- see temporal_host.hpp.
#include "temporal_host.hpp"

#include <cmath>
#include <cstring>

namespace srt {
namespace temporal {

srt_temporal_params DefaultParams() {
  srt_temporal_params p;
  p.max_history = 32;
  p.depth_tol = 0.05f;
  p.normal_min = 0.9f;
  return p;
}

int ValidateParams(const srt_temporal_params* p) {
  if (!p) return SRT_ERR_INVALID;
  if (p->max_history < 1 || p->max_history > (uint32_t)SRT_TEMPORAL_MAX_HISTORY) return SRT_ERR_INVALID;
  if (!std::isfinite(p->depth_tol) || !(p->depth_tol > 0.0f)) return SRT_ERR_INVALID;
  if (!std::isfinite(p->normal_min) || p->normal_min < -1.0f || p->normal_min > 1.0f) return SRT_ERR_INVALID;
  return SRT_OK;
}

int PlanBuffers(int width, int height, Sizes* out) {
  if (!out) return SRT_ERR_INVALID;
  *out = Sizes();
  if (width < 1 || height < 1) return SRT_ERR_INVALID;
  const uint64_t pixels = (uint64_t)width * (uint64_t)height;
  if (width > kMaxDim || height > kMaxDim || pixels > kMaxPixels) return SRT_ERR_LIMIT;
  out->pixels = pixels;
  out->color_bytes = (size_t)pixels * 16;
  out->guide_bytes = (size_t)pixels * 16;
  out->id_bytes = (size_t)pixels * 4;
  out->scratch_bytes = 2 * (out->color_bytes + out->guide_bytes + out->id_bytes);
  out->grid_x = (unsigned)((width + kRowW - 1) / kRowW);
  out->grid_y = (unsigned)((height + kRowH - 1) / kRowH);
  return SRT_OK;
}

void Reset(History* h) {
  h->valid = false;
  h->frames = 0;
}

void Advance(History* h, const srt_temporal_camera& cam) {
  h->read ^= 1;
  h->valid = true;
  h->prev = cam;
  if (h->frames < 0x7FFFFFFFu) ++h->frames;
}

// ---- moving models ----

namespace {

bool AffineFinite(const float m[16]) {
  for (int k = 0; k < 16; ++k)
    if (!std::isfinite(m[k])) return false;
  return m[3] == 0.0f && m[7] == 0.0f && m[11] == 0.0f && m[15] == 1.0f;
}

}  // namespace

int ValidateModels(const srt_temporal_model* models, uint32_t n) {
  if (n > kMaxModels) return SRT_ERR_LIMIT;
  if (n && !models) return SRT_ERR_INVALID;
  for (uint32_t r = 0; r < n; ++r)
    if (!AffineFinite(models[r].world_to_model) || !AffineFinite(models[r].model_to_world)) return SRT_ERR_INVALID;
  return SRT_OK;
}

int ModelFromFrame(const float frame[16], srt_temporal_model* out) {
  if (!frame || !out || !AffineFinite(frame)) return SRT_ERR_INVALID;
  // element (row i, column k) of the column-major frame
  double a[3][3], t[3];
  for (int i = 0; i < 3; ++i) {
    for (int k = 0; k < 3; ++k) a[i][k] = (double)frame[4 * k + i];
    t[i] = (double)frame[12 + i];
  }
  double c[3][3];  // cofactors: the inverse is their transpose over the determinant
  for (int i = 0; i < 3; ++i)
    for (int k = 0; k < 3; ++k) {
      const int i1 = (i + 1) % 3, i2 = (i + 2) % 3, k1 = (k + 1) % 3, k2 = (k + 2) % 3;
      c[i][k] = a[i1][k1] * a[i2][k2] - a[i1][k2] * a[i2][k1];
    }
  const double det = a[0][0] * c[0][0] + a[0][1] * c[0][1] + a[0][2] * c[0][2];
  if (!(det != 0.0) || !std::isfinite(det)) return SRT_ERR_INVALID;
  float inv[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1};
  for (int i = 0; i < 3; ++i) {
    double ti = 0.0;
    for (int k = 0; k < 3; ++k) {
      const double e = c[k][i] / det;
      inv[4 * k + i] = (float)e;
      ti -= e * t[k];
    }
    inv[12 + i] = (float)ti;
  }
  if (!AffineFinite(inv)) return SRT_ERR_INVALID;
  std::memcpy(out->world_to_model, frame, sizeof out->world_to_model);
  std::memcpy(out->model_to_world, inv, sizeof out->model_to_world);
  return SRT_OK;
}

int SetModels(Poses* p, const srt_temporal_model* models, uint32_t n) {
  if (!p) return SRT_ERR_INVALID;
  if (int rc = ValidateModels(models, n)) return rc;
  if (n) p->cur.assign(models, models + n);
  else p->cur.clear();
  return SRT_OK;
}

void ComposeMotion(const srt_temporal_model& pa, const srt_temporal_model& qb, float m[12]) {
  const float* a = pa.model_to_world;
  const float* b = qb.world_to_model;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 4; ++j) {
      float e = (a[i] * b[4 * j] + a[4 + i] * b[4 * j + 1]) + a[8 + i] * b[4 * j + 2];
      if (j == 3) e = e + a[12 + i];
      m[4 * i + j] = e;
    }
}

MotionRecord MotionOf(const Poses& p, uint32_t r) {
  MotionRecord rec;
  std::memset(&rec, 0, sizeof rec);
  rec.m[0] = rec.m[5] = rec.m[10] = 1.0f;
  if (r < p.prev.size() && r < p.cur.size() && std::memcmp(&p.prev[r], &p.cur[r], sizeof(srt_temporal_model)) != 0) {
    ComposeMotion(p.prev[r], p.cur[r], rec.m);
    rec.moving = 1;
  }
  return rec;
}

uint32_t FillChunk(const Poses& p, uint32_t first, MotionChunk* out) {
  std::memset(out, 0, sizeof *out);
  const uint32_t n = (uint32_t)p.cur.size();
  uint32_t k = 0;
  for (; k < kUploadChunk && first + k < n; ++k) out->r[k] = MotionOf(p, first + k);
  return k;
}

void AdvancePoses(Poses* p) {
  p->prev = p->cur;
}

void ResetPoses(Poses* p) {
  p->prev.clear();
}

// ---- deforming meshes ----

int ValidateMesh(const srt_triangle* tris, uint32_t n_tris, uint32_t n_verts) {
  if (n_tris >= kMaxMesh || n_verts >= kMaxMesh) return SRT_ERR_LIMIT;
  if (n_tris && (!tris || n_verts == 0)) return SRT_ERR_INVALID;
  return SRT_OK;
}

int AttachMesh(Mesh* m, const srt_triangle* tris, uint32_t n_tris, uint32_t n_verts) {
  if (int rc = ValidateMesh(tris, n_tris, n_verts)) return rc;
  if (!m) return SRT_ERR_INVALID;
  *m = Mesh();
  if (n_tris) {
    m->n_tris = n_tris;
    m->n_verts = n_verts;
  }
  return SRT_OK;
}

int SetVertices(Mesh* m, const void* verts_dev, uint32_t n_verts) {
  if (reinterpret_cast<uintptr_t>(verts_dev) % 16 != 0) return SRT_ERR_INVALID;
  if (!m || m->n_tris == 0 || n_verts != m->n_verts) return SRT_ERR_INVALID;
  m->verts = verts_dev;
  if (!verts_dev) m->has_prev = false;
  return SRT_OK;
}

void AdvanceMesh(Mesh* m) {
  if (DeformRuns(*m)) m->has_prev = true;
}

void ResetMesh(Mesh* m) {
  m->has_prev = false;
}

namespace {

// rows of a column-major affine matrix: row i = (a[i], a[4 + i], a[8 + i], a[12 + i])
void Rows(const float a[16], float rows[12]) {
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 4; ++j) rows[4 * i + j] = a[4 * j + i];
}

}  // namespace

DeformRecord DeformOf(const Poses& p, uint32_t r) {
  DeformRecord rec;
  std::memset(&rec, 0, sizeof rec);
  if (r >= p.cur.size()) return rec;
  Rows(p.cur[r].world_to_model, rec.w2m);
  Rows(r < p.prev.size() ? p.prev[r].model_to_world : p.cur[r].model_to_world, rec.a);
  return rec;
}

uint32_t FillDeformChunk(const Poses& p, uint32_t first, DeformChunk* out) {
  std::memset(out, 0, sizeof *out);
  const uint32_t n = (uint32_t)p.cur.size();
  uint32_t k = 0;
  for (; k < kUploadChunk && first + k < n; ++k) out->r[k] = DeformOf(p, first + k);
  return k;
}

// ---- luminance moments ----

void EnableMoments(Moments* m) {
  if (m->enabled) return;
  m->enabled = true;
  m->valid = false;
}

void AdvanceMoments(Moments* m, bool with_moments) {
  m->valid = m->enabled && with_moments;
}

void ResetMoments(Moments* m) {
  m->valid = false;
}

}  // namespace temporal
}  // namespace srt
