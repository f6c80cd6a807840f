// surface_host.cpp -- see surface_host.hpp.
#include "surface_host.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace srt {
namespace surface {

namespace {

float AsFloat(uint32_t u) {
  float f;
  std::memcpy(&f, &u, 4);
  return f;
}

int Fail(std::string* err, const std::string& msg, int rc = SRT_ERR_INVALID) {
  if (err) *err = msg;
  return rc;
}

}  // namespace

int BuildLayout(const srt_bvh_record* bvhs, uint32_t n_bvhs, const srt_material_obj* mats, const float* tex_albedo,
                uint32_t n_mats, const srt_triangle* tris, uint32_t n_tris, const srt_vertex* verts, uint32_t n_verts,
                Layout* out, std::string* err) {
  if (!out || (n_bvhs && !bvhs) || (n_mats && !mats) || (n_tris && !tris) || (n_verts && !verts))
    return Fail(err, "srt_surface_create: null argument");
  if (n_bvhs == 0) return Fail(err, "srt_surface_create: scene needs at least one BVH record");
  for (uint32_t t = 0; t < n_tris; ++t) {
    const srt_triangle& tr = tris[t];
    if (tr.v0_idx >= n_verts || tr.v1_idx >= n_verts || tr.v2_idx >= n_verts)
      return Fail(err, "srt_surface_create: triangle " + std::to_string(t) + " has a vertex index out of range");
    if (tr.material_idx >= n_mats)
      return Fail(err, "srt_surface_create: triangle " + std::to_string(t) + " has a material index out of range");
  }
  *out = Layout();
  out->n_bvhs = n_bvhs;
  out->n_tris = n_tris;
  out->n_mats = n_mats;
  out->frames.assign(16 * ((size_t)n_bvhs + 1), 0.0f);
  for (uint32_t b = 0; b < n_bvhs; ++b) std::memcpy(&out->frames[16 * (size_t)b], bvhs[b].frame, 16 * sizeof(float));
  out->tris.assign(4 * (size_t)std::max(n_tris, 1u), F4{0, 0, 0, 0});
  for (uint32_t t = 0; t < n_tris; ++t) {
    const srt_triangle& tr = tris[t];
    const srt_vertex &a = verts[tr.v0_idx], &b = verts[tr.v1_idx], &c = verts[tr.v2_idx];
    float e1[3], e2[3];
    for (int k = 0; k < 3; ++k) {
      e1[k] = b.vertex[k] - a.vertex[k];
      e2[k] = c.vertex[k] - a.vertex[k];
    }
    F4* r = &out->tris[4 * (size_t)t];
    r[0] = F4{a.vertex[0], a.vertex[1], a.vertex[2], e1[0]};
    r[1] = F4{e1[1], e1[2], e2[0], e2[1]};
    r[2] = F4{e2[2], AsFloat(tr.material_idx), a.texture[0], a.texture[1]};
    r[3] = F4{b.texture[0], b.texture[1], c.texture[0], c.texture[1]};
  }
  out->mats.assign(std::max(n_mats, 1u), F4{0, 0, 0, 0});
  for (uint32_t m = 0; m < n_mats; ++m) {
    const srt_material_obj& mo = mats[m];
    if (mo.use_texture == 0)
      out->mats[m] = F4{mo.diffuse[0], mo.diffuse[1], mo.diffuse[2], AsFloat(0u)};
    else if (tex_albedo)
      out->mats[m] = F4{tex_albedo[3 * (size_t)m], tex_albedo[3 * (size_t)m + 1], tex_albedo[3 * (size_t)m + 2], AsFloat(0u)};
    else
      out->mats[m] = F4{AsFloat(mo.handle[0]), AsFloat(mo.handle[1]), 0.0f, AsFloat(1u)};
  }
  return SRT_OK;
}

int PackTextures(const srt_texture* textures, uint32_t n, TexturePack* out, std::string* err) {
  if (!out || (n && !textures)) return Fail(err, "srt_surface_upload_textures: null argument");
  uint64_t total = 0;
  std::vector<uint32_t> info(4 * (size_t)std::max(n, 1u), 0u);
  for (uint32_t i = 0; i < n; ++i) {
    const srt_texture& t = textures[i];
    if (!t.texels || t.width <= 0 || t.height <= 0 || t.channels < 1 || t.channels > 4)
      return Fail(err, "texture " + std::to_string(i) + ": bad size, channel count or texel pointer");
    info[4 * (size_t)i + 0] = (uint32_t)total;
    info[4 * (size_t)i + 1] = (uint32_t)t.width;
    info[4 * (size_t)i + 2] = (uint32_t)t.height;
    total += (uint64_t)t.width * (uint64_t)t.height;
    if (total >= (1ull << 32)) return Fail(err, "textures hold more than 2^32 texels", SRT_ERR_LIMIT);
  }
  out->n = n;
  out->info = std::move(info);
  out->texels.assign(std::max<size_t>((size_t)total, 1), 0u);
  // GL_RED reads (r, 0, 0), a 2-channel file (r, g, 0); the kernel reads a channel as c / 255
  for (uint32_t i = 0; i < n; ++i) {
    const srt_texture& t = textures[i];
    const size_t m = (size_t)t.width * (size_t)t.height, first = out->info[4 * (size_t)i];
    for (size_t k = 0; k < m; ++k) {
      const uint8_t* p = t.texels + k * (size_t)t.channels;
      uint32_t v[3] = {0u, 0u, 0u};
      for (int ch = 0; ch < t.channels && ch < 3; ++ch) v[ch] = p[ch];
      if (t.channels == 2) v[2] = 0u;
      out->texels[first + k] = v[0] | (v[1] << 8) | (v[2] << 16);
    }
  }
  return SRT_OK;
}

bool ValidFloor(float albedo_floor) { return std::isfinite(albedo_floor) && albedo_floor > 0.0f; }

}  // namespace surface
}  // namespace srt
