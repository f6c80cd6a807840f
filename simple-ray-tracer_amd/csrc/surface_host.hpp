// surface_host.hpp -- host-only parts of the surface-attribute stage (include/srt_surface.h): validation of the
// std430 scene arrays, their packing for surface_shade_kernel and the RGBA8 texture pack.  No device, no HIP
// header: tests/cpp/test_surface_host.cpp links surface_host.cpp alone.
#pragma once

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/srt_surface.h"

namespace srt {
namespace surface {

struct F4 {
  float x, y, z, w;
};

constexpr int kBlock = 256;  // lanes per block of surface_shade_kernel

// Device arrays of a scene, every record a whole number of 16-B words.
//   frames: 16 floats per BVH record (column-major, as srt_bvh_record.frame), n_bvhs + 1 records: the last is
//           zeros, read for a hit whose bvh is at or past bvh_count or n_bvhs.
//   tris:   64 B per triangle in input order: (v0 | e1.x) (e1.yz | e2.xy) (e2.z, material_idx, uv0) (uv1 | uv2)
//           with e1 = v1 - v0, e2 = v2 - v0 (the fp32 subtractions IntersectsTriangle makes).
//   mats:   16 B per material.  w == 0: (albedo, 0) -- diffuse, or the material's tex_albedo when one was given;
//           w == 1: (handle[0], handle[1], 0, 1) as bits -- the texture is sampled at the hit's uv.
struct Layout {
  std::vector<float> frames;
  std::vector<F4> tris, mats;
  uint32_t n_bvhs = 0, n_tris = 0, n_mats = 0;
};

// SRT_OK, or SRT_ERR_INVALID with a message in *err: a NULL array with a non-zero count, no BVH record, a
// triangle's vertex or material index out of range.
int BuildLayout(const srt_bvh_record* bvhs, uint32_t n_bvhs, const srt_material_obj* mats, const float* tex_albedo,
                uint32_t n_mats, const srt_triangle* tris, uint32_t n_tris, const srt_vertex* verts, uint32_t n_verts,
                Layout* out, std::string* err);

// The textures of srt_surface_upload_textures: texels r | g << 8 | b << 16 of all textures back to back, and per
// texture (first texel, width, height, 0).  Both arrays hold at least one (zero) entry.
struct TexturePack {
  std::vector<uint32_t> texels;
  std::vector<uint32_t> info;  // 4 per texture
  uint32_t n = 0;
};
// SRT_OK; SRT_ERR_INVALID: NULL `textures` with n > 0, a NULL texel pointer, a size < 1, channels outside 1..4;
// SRT_ERR_LIMIT: 2^32 texels or more in all.
int PackTextures(const srt_texture* textures, uint32_t n, TexturePack* out, std::string* err);

// srt_denoise_run_albedo's floor: finite and > 0.
bool ValidFloor(float albedo_floor);

}  // namespace surface
}  // namespace srt
