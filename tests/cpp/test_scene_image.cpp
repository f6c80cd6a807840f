// What srt_upload_scene sends to the device (csrc/scene_image.cpp: the scene policy and the device arrays) as
// a stand-alone program, meant for AddressSanitizer + UBSan on the CPU (no device, no HIP runtime):
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -I/opt/rocm/include
//       -D__HIP_PLATFORM_AMD__ tests/cpp/test_scene_image.cpp simple-ray-tracer_amd/csrc/scene_image.cpp
//       simple-ray-tracer_amd/csrc/scene_layout.cpp simple-ray-tracer_amd/csrc/scene.cpp -lz -pthread -o test_scene_image
//   ./test_scene_image tests/golden/objects/Rubik/Rubik.obj
// Hand-made trees of 3 to 15 nodes and Rubik's, each under every layout choice; the arrays' properties, and
// their bytes against fingerprints taken from the upload code before it moved here.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <set>
#include <string>
#include <vector>

#include "../../simple-ray-tracer_amd/csrc/scene_image.hpp"
#include "../../simple-ray-tracer_amd/csrc/scene_layout.hpp"

static std::string g_error;
namespace srt {
void SetError(const std::string& msg) { g_error = msg; }  // (the library's lives in context.cpp, with HIP)
}  // namespace srt

static int g_fail = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      std::fprintf(stderr, "%s:%d: CHECK(%s) failed [%s]\n", __FILE__, __LINE__, #cond, g_case.c_str()); \
      ++g_fail;                                                            \
    }                                                                      \
  } while (0)
static std::string g_case;

// ---- cases: the inputs and the environment of every fingerprinted upload ------------------------------------
struct Case {
  std::string name;
  std::vector<srt_bvh_node> nodes;
  std::vector<srt_bvh_record> bvhs;
  std::vector<srt_material_obj> mats;
  std::vector<float> albedo;  // 3 per material; empty: none given, so materials with use_texture sample
  std::vector<srt_triangle> tris;
  std::vector<srt_vertex> verts;
  int treelet_depth;
};

static srt_bvh_node Node(uint32_t i, uint32_t first, uint32_t count) {
  srt_bvh_node n{};
  for (int k = 0; k < 3; ++k) {
    n.min_bounds[k] = -1.0f - 0.25f * (float)i - (float)k;
    n.max_bounds[k] = 0.5f + 0.125f * (float)i + (float)k;
  }
  n.first_child_or_prim_index = first;
  n.prim_count = count;
  return n;
}
static srt_bvh_record Record(uint32_t root) {
  srt_bvh_record r{};
  r.first_index = root;
  for (int i = 0; i < 4; ++i) r.frame[5 * i] = 1.0f;
  return r;
}
// A full binary tree in breadth-first order (node i's children are 2i+1 and 2i+2); leaf k holds sizes[k % n] triangles.
static void FullTree(Case* c, int levels, const std::vector<uint32_t>& sizes) {
  const uint32_t n = (2u << levels) - 1, internal = n / 2;
  uint32_t t = 0;
  for (uint32_t i = 0; i < n; ++i) {
    const uint32_t sz = sizes[(i - internal) % sizes.size()];
    c->nodes.push_back(i < internal ? Node(i, 2 * i + 1, 0) : Node(i, t, sz));
    if (i >= internal) t += sz;
  }
}
// Triangles 0 .. n-1 over 2n + 1 vertices (the last index of some is past the array: such a vertex reads
// zero), material t mod (n_mats + 2) (the last two are out of range), and three materials: plain, textured
// (handle 7), and one with exponent 0.
static void Geometry(Case* c, uint32_t n_tris, bool albedo) {
  for (uint32_t v = 0; v < 2 * n_tris + 1; ++v) {
    srt_vertex x{};
    for (int k = 0; k < 3; ++k) x.vertex[k] = 0.5f * (float)v - 1.75f * (float)k + 0.0625f * (float)((v * 7 + k) % 5);
    x.texture[0] = 0.03125f * (float)(v % 32);
    x.texture[1] = 1.0f - 0.015625f * (float)(v % 64);
    c->verts.push_back(x);
  }
  for (uint32_t t = 0; t < n_tris; ++t) c->tris.push_back({2 * t, 2 * t + 1, t % 5 == 4 ? 2 * t + 9 : 2 * t + 2, t % 5});
  for (uint32_t m = 0; m < 3; ++m) {
    srt_material_obj o{};
    for (int k = 0; k < 3; ++k) {
      o.diffuse[k] = 0.25f * (float)(m + 1) + 0.0625f * (float)k;
      o.specular[k] = 0.125f * (float)(k + 1) * (float)(m + 1);
    }
    o.specular_ex = m == 2 ? 0.0f : 10.0f * (float)(m + 1);
    o.use_texture = m == 1;
    o.handle[0] = 7;
    c->mats.push_back(o);
    if (albedo)
      for (int k = 0; k < 3; ++k) c->albedo.push_back(0.75f - 0.125f * (float)k);
  }
}
static uint32_t CountTris(const Case& c) {
  uint32_t n = 0;
  for (const auto& nd : c.nodes)
    if (nd.prim_count && nd.prim_count < 1000) n = std::max(n, nd.first_child_or_prim_index + nd.prim_count);
  return n;
}
static std::vector<Case> HandMadeCases() {
  std::vector<Case> cases(4);
  cases[0].name = "t3";  // one pair
  FullTree(&cases[0], 1, {1});
  cases[0].bvhs = {Record(0)};
  cases[1].name = "t7shared";  // two records, the second into the first's tree
  FullTree(&cases[1], 2, {1, 2});
  cases[1].bvhs = {Record(0), Record(2)};
  cases[2].name = "t9stray";  // two nodes no traversal reaches, holding garbage
  FullTree(&cases[2], 2, {2, 1, 1});
  cases[2].nodes.push_back(Node(7, 0xDEADBEEFu, 0));
  cases[2].nodes.push_back(Node(8, 0xDEADBEEFu, 77777));
  cases[2].bvhs = {Record(0)};
  cases[3].name = "t15tex";  // mixed leaves, and no albedo array: the textured material samples
  FullTree(&cases[3], 3, {1, 2, 4, 1, 1, 2, 3});
  cases[3].bvhs = {Record(0)};
  for (size_t i = 0; i < cases.size(); ++i) {
    Geometry(&cases[i], CountTris(cases[i]), i != 3);
    cases[i].treelet_depth = 1;
  }
  return cases;
}
// The layout choices of one upload, set through the environment ChooseScenePolicy reads.  `pad` appends
// 32,768 unreachable nodes (1 MB: below that size no top region is chosen).
struct Config { int pad, align, tri, top; };
static std::vector<Config> Configs() {
  std::vector<Config> v;
  for (int pad = 0; pad < 2; ++pad)
    for (int align = 0; align < 2; ++align)
      for (int tri = 0; tri < 2; ++tri)
        for (int top = 0; top <= (pad ? 3 : 0); top += 3) v.push_back({pad, align, tri, top});
  return v;
}
static std::string Tag(const Case& c, const Config& g) {
  return c.name + "/p" + std::to_string(g.pad) + "a" + std::to_string(g.align) + "t" + std::to_string(g.tri) + "d" +
         std::to_string(g.top);
}
static Case Apply(const Case& c, const Config& g) {
  setenv("SRT_NODE_ALIGN", g.align ? "1" : "0", 1);
  setenv("SRT_TRI_ALIGN", g.tri ? "1" : "0", 1);
  setenv("SRT_TOP_DEPTH", g.top ? "3" : "0", 1);
  setenv("SRT_GLOBAL_FUSED_MODE", "1", 1);
  Case p = c;
  if (g.pad) p.nodes.resize(p.nodes.size() + 32768, srt_bvh_node{});
  return p;
}
static unsigned long long Fnv(const void* data, size_t bytes) {  // FNV-1a, 64 bit
  unsigned long long h = 0xcbf29ce484222325ull;
  for (size_t i = 0; i < bytes; ++i) h = (h ^ static_cast<const unsigned char*>(data)[i]) * 0x100000001b3ull;
  return h;
}
// ---- end of cases --------------------------------------------------------------------------------------------

// The product build's constants (kernels.hpp, traversal.hpp, pool.hpp at their defaults).
static constexpr srt::BuildConsts kProduct = {1024, 256, 5, 16, 8, false, 24 * 128 + 256, 29, 64 * 14, 2, 3, 255};

// Fingerprints {nodes, treelet copy, treelet roots, materials, triangles, uvs} of the arrays srt_upload_scene
// sent before this code moved out of pathtrace.hip: taken from commit df7079d's srt_upload_scene, its body
// compiled unchanged in a host program with hipMalloc as malloc and the copies as memcpy, on these cases.
struct Parent { const char* tag; unsigned long long fp[6]; };
static const Parent kParent[] = {
    {"t3/p0a0t0d0", {0xb058686231c53540ull, 0xcbf29ce484222325ull, 0xcbf29ce484222325ull, 0x760802eaab91a5d5ull, 0x2f5b259348c91cd7ull, 0xcbf29ce484222325ull}},
    {"t3/p0a0t1d0", {0xb058686231c53540ull, 0xcbf29ce484222325ull, 0xcbf29ce484222325ull, 0x760802eaab91a5d5ull, 0x2f5b259348c91cd7ull, 0xcbf29ce484222325ull}},
    {"t3/p0a1t0d0", {0xb058686231c53540ull, 0xcbf29ce484222325ull, 0xcbf29ce484222325ull, 0x760802eaab91a5d5ull, 0x2f5b259348c91cd7ull, 0xcbf29ce484222325ull}},
    {"t3/p0a1t1d0", {0xb058686231c53540ull, 0xcbf29ce484222325ull, 0xcbf29ce484222325ull, 0x760802eaab91a5d5ull, 0x2f5b259348c91cd7ull, 0xcbf29ce484222325ull}},
    {"t3/p1a0t0d0", {0xb058686231c53540ull, 0xcbf29ce484222325ull, 0xcbf29ce484222325ull, 0x760802eaab91a5d5ull, 0x2f5b259348c91cd7ull, 0xcbf29ce484222325ull}},
    {"t3/p1a0t0d3", {0xb058686231c53540ull, 0xcbf29ce484222325ull, 0xcbf29ce484222325ull, 0x760802eaab91a5d5ull, 0x2f5b259348c91cd7ull, 0xcbf29ce484222325ull}},
    {"t3/p1a0t1d0", {0xb058686231c53540ull, 0xcbf29ce484222325ull, 0xcbf29ce484222325ull, 0x760802eaab91a5d5ull, 0x2f5b259348c91cd7ull, 0xcbf29ce484222325ull}},
    {"t3/p1a0t1d3", {0xb058686231c53540ull, 0xcbf29ce484222325ull, 0xcbf29ce484222325ull, 0x760802eaab91a5d5ull, 0x2f5b259348c91cd7ull, 0xcbf29ce484222325ull}},
    {"t3/p1a1t0d0", {0xb058686231c53540ull, 0xcbf29ce484222325ull, 0xcbf29ce484222325ull, 0x760802eaab91a5d5ull, 0x2f5b259348c91cd7ull, 0xcbf29ce484222325ull}},
    {"t3/p1a1t0d3", {0xb058686231c53540ull, 0xcbf29ce484222325ull, 0xcbf29ce484222325ull, 0x760802eaab91a5d5ull, 0x2f5b259348c91cd7ull, 0xcbf29ce484222325ull}},
    {"t3/p1a1t1d0", {0xb058686231c53540ull, 0xcbf29ce484222325ull, 0xcbf29ce484222325ull, 0x760802eaab91a5d5ull, 0x2f5b259348c91cd7ull, 0xcbf29ce484222325ull}},
    {"t3/p1a1t1d3", {0xb058686231c53540ull, 0xcbf29ce484222325ull, 0xcbf29ce484222325ull, 0x760802eaab91a5d5ull, 0x2f5b259348c91cd7ull, 0xcbf29ce484222325ull}},
    {"t7shared/p0a0t0d0", {0xe074f2adb185db35ull, 0x902a48e5fd3a48b2ull, 0xedd2191df40efcd3ull, 0x760802eaab91a5d5ull, 0x78c2c18bad5e7ce5ull, 0xcbf29ce484222325ull}},
    {"t7shared/p0a0t1d0", {0x08106e70ce140f02ull, 0x56fd5d0d0e3f70ddull, 0xedd2191df40efcd3ull, 0x760802eaab91a5d5ull, 0x6ab38e7c642e90a5ull, 0xcbf29ce484222325ull}},
    {"t7shared/p0a1t0d0", {0xe074f2adb185db35ull, 0x902a48e5fd3a48b2ull, 0xedd2191df40efcd3ull, 0x760802eaab91a5d5ull, 0x78c2c18bad5e7ce5ull, 0xcbf29ce484222325ull}},
    {"t7shared/p0a1t1d0", {0x08106e70ce140f02ull, 0x56fd5d0d0e3f70ddull, 0xedd2191df40efcd3ull, 0x760802eaab91a5d5ull, 0x6ab38e7c642e90a5ull, 0xcbf29ce484222325ull}},
    {"t7shared/p1a0t0d0", {0x0d7052eecec5db35ull, 0x50614fc949ba48b2ull, 0xedd2191df40efcd3ull, 0x760802eaab91a5d5ull, 0x78c2c18bad5e7ce5ull, 0xcbf29ce484222325ull}},
    {"t7shared/p1a0t0d3", {0x0d7052eecec5db35ull, 0x50614fc949ba48b2ull, 0xedd2191df40efcd3ull, 0x760802eaab91a5d5ull, 0x78c2c18bad5e7ce5ull, 0xcbf29ce484222325ull}},
    {"t7shared/p1a0t1d0", {0xb3eada9aae940f02ull, 0xbe3061c6157f70ddull, 0xedd2191df40efcd3ull, 0x760802eaab91a5d5ull, 0x6ab38e7c642e90a5ull, 0xcbf29ce484222325ull}},
    {"t7shared/p1a0t1d3", {0xb3eada9aae940f02ull, 0xbe3061c6157f70ddull, 0xedd2191df40efcd3ull, 0x760802eaab91a5d5ull, 0x6ab38e7c642e90a5ull, 0xcbf29ce484222325ull}},
    {"t7shared/p1a1t0d0", {0x0d7052eecec5db35ull, 0x50614fc949ba48b2ull, 0xedd2191df40efcd3ull, 0x760802eaab91a5d5ull, 0x78c2c18bad5e7ce5ull, 0xcbf29ce484222325ull}},
    {"t7shared/p1a1t0d3", {0x0d7052eecec5db35ull, 0x50614fc949ba48b2ull, 0xedd2191df40efcd3ull, 0x760802eaab91a5d5ull, 0x78c2c18bad5e7ce5ull, 0xcbf29ce484222325ull}},
    {"t7shared/p1a1t1d0", {0xb3eada9aae940f02ull, 0xbe3061c6157f70ddull, 0xedd2191df40efcd3ull, 0x760802eaab91a5d5ull, 0x6ab38e7c642e90a5ull, 0xcbf29ce484222325ull}},
    {"t7shared/p1a1t1d3", {0xb3eada9aae940f02ull, 0xbe3061c6157f70ddull, 0xedd2191df40efcd3ull, 0x760802eaab91a5d5ull, 0x6ab38e7c642e90a5ull, 0xcbf29ce484222325ull}},
    {"t9stray/p0a0t0d0", {0x6f565d4dc55e12d3ull, 0x7fe27bc530b49639ull, 0xe7d2bb2230684e33ull, 0x760802eaab91a5d5ull, 0x78c2c18bad5e7ce5ull, 0xcbf29ce484222325ull}},
    {"t9stray/p0a0t1d0", {0x3e49bd9739237de3ull, 0x0f858a27861afa71ull, 0xe7d2bb2230684e33ull, 0x760802eaab91a5d5ull, 0x2a8652e9f473fda5ull, 0xcbf29ce484222325ull}},
    {"t9stray/p0a1t0d0", {0x66b26c52be1ffc29ull, 0xcc7f46ffe9ca0983ull, 0x6dbcc93f4ce5ef17ull, 0x760802eaab91a5d5ull, 0x78c2c18bad5e7ce5ull, 0xcbf29ce484222325ull}},
    {"t9stray/p0a1t1d0", {0x6c1aac59a6dcc861ull, 0x43d0320d4514fb53ull, 0x6dbcc93f4ce5ef17ull, 0x760802eaab91a5d5ull, 0x2a8652e9f473fda5ull, 0xcbf29ce484222325ull}},
    {"t9stray/p1a0t0d0", {0x6f565d4dc55e12d3ull, 0x7fe27bc530b49639ull, 0xe7d2bb2230684e33ull, 0x760802eaab91a5d5ull, 0x78c2c18bad5e7ce5ull, 0xcbf29ce484222325ull}},
    {"t9stray/p1a0t0d3", {0x6f565d4dc55e12d3ull, 0x7fe27bc530b49639ull, 0xe7d2bb2230684e33ull, 0x760802eaab91a5d5ull, 0x78c2c18bad5e7ce5ull, 0xcbf29ce484222325ull}},
    {"t9stray/p1a0t1d0", {0x3e49bd9739237de3ull, 0x0f858a27861afa71ull, 0xe7d2bb2230684e33ull, 0x760802eaab91a5d5ull, 0x2a8652e9f473fda5ull, 0xcbf29ce484222325ull}},
    {"t9stray/p1a0t1d3", {0x3e49bd9739237de3ull, 0x0f858a27861afa71ull, 0xe7d2bb2230684e33ull, 0x760802eaab91a5d5ull, 0x2a8652e9f473fda5ull, 0xcbf29ce484222325ull}},
    {"t9stray/p1a1t0d0", {0x66b26c52be1ffc29ull, 0xcc7f46ffe9ca0983ull, 0x6dbcc93f4ce5ef17ull, 0x760802eaab91a5d5ull, 0x78c2c18bad5e7ce5ull, 0xcbf29ce484222325ull}},
    {"t9stray/p1a1t0d3", {0x66b26c52be1ffc29ull, 0xcc7f46ffe9ca0983ull, 0x6dbcc93f4ce5ef17ull, 0x760802eaab91a5d5ull, 0x78c2c18bad5e7ce5ull, 0xcbf29ce484222325ull}},
    {"t9stray/p1a1t1d0", {0x6c1aac59a6dcc861ull, 0x43d0320d4514fb53ull, 0x6dbcc93f4ce5ef17ull, 0x760802eaab91a5d5ull, 0x2a8652e9f473fda5ull, 0xcbf29ce484222325ull}},
    {"t9stray/p1a1t1d3", {0x6c1aac59a6dcc861ull, 0x43d0320d4514fb53ull, 0x6dbcc93f4ce5ef17ull, 0x760802eaab91a5d5ull, 0x2a8652e9f473fda5ull, 0xcbf29ce484222325ull}},
    {"t15tex/p0a0t0d0", {0x9222481014c67a85ull, 0x6354ff06029bf9dfull, 0xe692e686efa6b28full, 0x65263c9151b7f440ull, 0x1796fe73945a2658ull, 0x9f45afbc94a42c3full}},
    {"t15tex/p0a0t1d0", {0xe6a39c1ceb3360a5ull, 0x48c28a607b23b33full, 0xe692e686efa6b28full, 0x65263c9151b7f440ull, 0x5ceec6a2a2bc9498ull, 0xc343f44ccf3f12bfull}},
    {"t15tex/p0a1t0d0", {0xb1c965af4491c97full, 0xe26251c9dc23f385ull, 0x6ca794615a766eebull, 0x65263c9151b7f440ull, 0x1796fe73945a2658ull, 0x9f45afbc94a42c3full}},
    {"t15tex/p0a1t1d0", {0x9e91887afa54e4e7ull, 0xa18ff254d554e52dull, 0x6ca794615a766eebull, 0x65263c9151b7f440ull, 0x5ceec6a2a2bc9498ull, 0xc343f44ccf3f12bfull}},
    {"t15tex/p1a0t0d0", {0x9222481014c67a85ull, 0x6354ff06029bf9dfull, 0xe692e686efa6b28full, 0x65263c9151b7f440ull, 0x1796fe73945a2658ull, 0x9f45afbc94a42c3full}},
    {"t15tex/p1a0t0d3", {0x9222481014c67a85ull, 0x6354ff06029bf9dfull, 0xe692e686efa6b28full, 0x65263c9151b7f440ull, 0x1796fe73945a2658ull, 0x9f45afbc94a42c3full}},
    {"t15tex/p1a0t1d0", {0xe6a39c1ceb3360a5ull, 0x48c28a607b23b33full, 0xe692e686efa6b28full, 0x65263c9151b7f440ull, 0x5ceec6a2a2bc9498ull, 0xc343f44ccf3f12bfull}},
    {"t15tex/p1a0t1d3", {0xe6a39c1ceb3360a5ull, 0x48c28a607b23b33full, 0xe692e686efa6b28full, 0x65263c9151b7f440ull, 0x5ceec6a2a2bc9498ull, 0xc343f44ccf3f12bfull}},
    {"t15tex/p1a1t0d0", {0xb1c965af4491c97full, 0xe26251c9dc23f385ull, 0x6ca794615a766eebull, 0x65263c9151b7f440ull, 0x1796fe73945a2658ull, 0x9f45afbc94a42c3full}},
    {"t15tex/p1a1t0d3", {0xb1c965af4491c97full, 0xe26251c9dc23f385ull, 0x6ca794615a766eebull, 0x65263c9151b7f440ull, 0x1796fe73945a2658ull, 0x9f45afbc94a42c3full}},
    {"t15tex/p1a1t1d0", {0x9e91887afa54e4e7ull, 0xa18ff254d554e52dull, 0x6ca794615a766eebull, 0x65263c9151b7f440ull, 0x5ceec6a2a2bc9498ull, 0xc343f44ccf3f12bfull}},
    {"t15tex/p1a1t1d3", {0x9e91887afa54e4e7ull, 0xa18ff254d554e52dull, 0x6ca794615a766eebull, 0x65263c9151b7f440ull, 0x5ceec6a2a2bc9498ull, 0xc343f44ccf3f12bfull}},
    {"rubik/p0a0t0d0", {0x1eb468fdc87ccd9full, 0x459da8fca37dfabcull, 0x1ee95705060eb426ull, 0xbf1a744cf19a29b9ull, 0x5cea06a4bda25a98ull, 0xcbf29ce484222325ull}},
    {"rubik/p0a0t1d0", {0x1eb468fdc87ccd9full, 0x459da8fca37dfabcull, 0x1ee95705060eb426ull, 0xbf1a744cf19a29b9ull, 0x5cea06a4bda25a98ull, 0xcbf29ce484222325ull}},
    {"rubik/p0a1t0d0", {0x61b3611ba72db79cull, 0xbf03043030968859ull, 0x10742a4eac27fb90ull, 0xbf1a744cf19a29b9ull, 0x5cea06a4bda25a98ull, 0xcbf29ce484222325ull}},
    {"rubik/p0a1t1d0", {0x61b3611ba72db79cull, 0xbf03043030968859ull, 0x10742a4eac27fb90ull, 0xbf1a744cf19a29b9ull, 0x5cea06a4bda25a98ull, 0xcbf29ce484222325ull}},
    {"rubik/p1a0t0d0", {0x1eb468fdc87ccd9full, 0x459da8fca37dfabcull, 0x1ee95705060eb426ull, 0xbf1a744cf19a29b9ull, 0x5cea06a4bda25a98ull, 0xcbf29ce484222325ull}},
    {"rubik/p1a0t0d3", {0x21d70892bfacb8afull, 0xa0581d1b336d2ff0ull, 0x9861209f4e38f18eull, 0xbf1a744cf19a29b9ull, 0x5cea06a4bda25a98ull, 0xcbf29ce484222325ull}},
    {"rubik/p1a0t1d0", {0x1eb468fdc87ccd9full, 0x459da8fca37dfabcull, 0x1ee95705060eb426ull, 0xbf1a744cf19a29b9ull, 0x5cea06a4bda25a98ull, 0xcbf29ce484222325ull}},
    {"rubik/p1a0t1d3", {0x21d70892bfacb8afull, 0xa0581d1b336d2ff0ull, 0x9861209f4e38f18eull, 0xbf1a744cf19a29b9ull, 0x5cea06a4bda25a98ull, 0xcbf29ce484222325ull}},
    {"rubik/p1a1t0d0", {0x61b3611ba72db79cull, 0xbf03043030968859ull, 0x10742a4eac27fb90ull, 0xbf1a744cf19a29b9ull, 0x5cea06a4bda25a98ull, 0xcbf29ce484222325ull}},
    {"rubik/p1a1t0d3", {0xe8f84399a14b0ce0ull, 0xd1b1594d48d5acc4ull, 0x1e6211238ee9bd01ull, 0xbf1a744cf19a29b9ull, 0x5cea06a4bda25a98ull, 0xcbf29ce484222325ull}},
    {"rubik/p1a1t1d0", {0x61b3611ba72db79cull, 0xbf03043030968859ull, 0x10742a4eac27fb90ull, 0xbf1a744cf19a29b9ull, 0x5cea06a4bda25a98ull, 0xcbf29ce484222325ull}},
    {"rubik/p1a1t1d3", {0xe8f84399a14b0ce0ull, 0xd1b1594d48d5acc4ull, 0x1e6211238ee9bd01ull, 0xbf1a744cf19a29b9ull, 0x5cea06a4bda25a98ull, 0xcbf29ce484222325ull}},
};

static uint32_t U32(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }
static bool Zero(const float4& v) { return U32(v.x) == 0 && U32(v.y) == 0 && U32(v.z) == 0 && U32(v.w) == 0; }
template <typename T>
static unsigned long long FnvOf(const std::vector<T>& v) { return Fnv(v.data(), v.size() * sizeof(T)); }

static int Build(const Case& c, const srt::ScenePolicy& policy, const srt::BuildConsts& k, srt::SceneImage* img,
                 std::vector<uint8_t>* reach, std::vector<std::pair<uint32_t, uint32_t>>* ranges) {
  int depth = 0;
  const int rc = srt::ValidateNodes(c.nodes.data(), (uint32_t)c.nodes.size(), (uint32_t)c.tris.size(), c.bvhs.data(),
                                    (uint32_t)c.bvhs.size(), &depth, ranges, reach);
  if (rc) return rc;
  const srt::SceneArrays in{c.bvhs.data(), (uint32_t)c.bvhs.size(), c.nodes.data(), (uint32_t)c.nodes.size(),
                            c.mats.data(), c.albedo.empty() ? nullptr : c.albedo.data(), (uint32_t)c.mats.size(),
                            c.tris.data(), (uint32_t)c.tris.size(), c.verts.data(), (uint32_t)c.verts.size()};
  srt::BuildSceneImage(in, depth, *ranges, *reach, policy, k, 0, img);
  return SRT_OK;
}

// The properties of one image.
static void CheckImage(const Case& c, const srt::ScenePolicy& policy, const srt::SceneImage& img,
                       const std::vector<uint8_t>& reach, const std::vector<std::pair<uint32_t, uint32_t>>& ranges) {
  const srt::BuildConsts& k = kProduct;
  const uint32_t n_tris = (uint32_t)c.tris.size(), n_mats = (uint32_t)c.mats.size();
  // triangle slots
  std::vector<uint32_t> tslot(n_tris);
  uint32_t n_tslots = n_tris;
  for (uint32_t t = 0; t < n_tris; ++t) tslot[t] = t;
  if (policy.tri_align) CHECK(srt::LayoutTris(c.nodes.data(), (uint32_t)c.nodes.size(), reach, n_tris, &tslot, &n_tslots));
  CHECK(img.n_tslots == n_tslots && img.tris.size() == 3 * ((size_t)n_tslots + k.tri_pad));
  // node records: input node i <-> slot s, walked from slot 0 and from every record's root
  // (two records sharing a pair: LayoutNodes declines, the input order stays and references are plain indices)
  const uint32_t ror = c.bvhs.size() == 1 ? 1u : 0u;
  CHECK(img.nodes.size() == 2 * ((size_t)img.n_slots + 1 + k.node_pad) && img.ref_or == ror && img.pairs_aligned);
  CHECK(ror || img.n_slots == c.nodes.size());
  std::set<uint32_t> slots;
  std::vector<std::pair<uint32_t, uint32_t>> st{{0u, 0u}};
  CHECK(img.bvhs.size() == c.bvhs.size() && img.bvh_tris.size() == c.bvhs.size());
  for (size_t b = 0; b < c.bvhs.size(); ++b) {
    st.push_back({c.bvhs[b].first_index, img.bvhs[b].first_index});
    CHECK(std::memcmp(img.bvhs[b].frame, c.bvhs[b].frame, sizeof(c.bvhs[b].frame)) == 0);
    if (ranges[b].first < ranges[b].second)
      CHECK(img.bvh_tris[b] == std::make_pair(tslot[ranges[b].first], tslot[ranges[b].second - 1] + 1));
  }
  size_t reached = 0;
  while (!st.empty()) {
    const auto [i, s] = st.back();
    st.pop_back();
    CHECK(s < img.n_slots && reach[i]);
    if (s >= img.n_slots) return;
    if (!slots.insert(s).second) continue;
    ++reached;
    const srt_bvh_node& n = c.nodes[i];
    const float4 lo = img.nodes[2 * (size_t)s + 2], hi = img.nodes[2 * (size_t)s + 3];
    CHECK(lo.x == n.min_bounds[0] && lo.y == n.min_bounds[1] && lo.z == n.min_bounds[2]);
    CHECK(hi.x == n.max_bounds[0] && hi.y == n.max_bounds[1] && hi.z == n.max_bounds[2] && U32(hi.w) == n.prim_count);
    if (n.prim_count) {
      CHECK(U32(lo.w) == tslot[n.first_child_or_prim_index]);
      continue;
    }
    const uint32_t ref = U32(lo.w) | ror, c0 = n.first_child_or_prim_index;
    CHECK(ref & 1u);
    st.push_back({c0, ref});
    st.push_back({c0 + 1, ref + 1});
    // the right-spine flag (an even reference): exactly where the right child's own pair is the next pair
    const bool flag = (U32(lo.w) & 1u) == 0;
    const bool next = ror && c.nodes[c0 + 1].prim_count == 0 && ref + 1 < img.n_slots &&
                      (U32(img.nodes[2 * (size_t)(ref + 1) + 2].w) | 1u) == ref + 2;
    CHECK(flag == next);
  }
  CHECK(reached == (size_t)std::count(reach.begin(), reach.end(), 1));  // one slot per reachable node
  CHECK(Zero(img.nodes[0]) && Zero(img.nodes[1]));
  for (uint32_t s = 0; s < img.n_slots + k.node_pad; ++s)  // unreachable nodes, alignment gaps, the pad
    if (!slots.count(s)) CHECK(Zero(img.nodes[2 * (size_t)s + 2]) && Zero(img.nodes[2 * (size_t)s + 3]));
  // the top region holds whole pairs from slot 1
  CHECK(img.n_top <= img.n_slots && (img.n_top == 0 || (img.n_top & 1u) == 1u) && (img.n_top > 0) == (img.top_depth > 0));
  CHECK(policy.top_depth > 0 || img.n_top == 0);
  // triangle records
  std::vector<uint8_t> used(n_tslots + k.tri_pad, 0);
  auto vert = [&](uint32_t i, int a) { return i < c.verts.size() ? c.verts[i].vertex[a] : 0.0f; };
  auto uv = [&](uint32_t i, int a) { return i < c.verts.size() ? c.verts[i].texture[a] : 0.0f; };
  CHECK(img.tri_uv.empty() == !img.sampled && (img.tri_uv.empty() || img.tri_uv.size() == 2 * (size_t)n_tslots));
  for (uint32_t t = 0; t < n_tris; ++t) {
    const srt_triangle& tr = c.tris[t];
    const size_t s = tslot[t];
    used[s] = 1;
    const float4 a = img.tris[3 * s], b = img.tris[3 * s + 1], d = img.tris[3 * s + 2];
    const float v0[3] = {vert(tr.v0_idx, 0), vert(tr.v0_idx, 1), vert(tr.v0_idx, 2)};
    CHECK(a.x == v0[0] && a.y == v0[1] && a.z == v0[2] && a.w == vert(tr.v1_idx, 0) - v0[0]);
    CHECK(b.x == vert(tr.v1_idx, 1) - v0[1] && b.y == vert(tr.v1_idx, 2) - v0[2] && b.z == vert(tr.v2_idx, 0) - v0[0] &&
          b.w == vert(tr.v2_idx, 1) - v0[1]);
    CHECK(d.x == vert(tr.v2_idx, 2) - v0[2] && U32(d.y) == std::min(tr.material_idx, n_mats) && U32(d.z) == t && U32(d.w) == 0);
    if (!img.tri_uv.empty()) {
      const float4 p = img.tri_uv[2 * s], q = img.tri_uv[2 * s + 1];
      CHECK(p.x == uv(tr.v0_idx, 0) && p.y == uv(tr.v0_idx, 1) && p.z == uv(tr.v1_idx, 0) && p.w == uv(tr.v1_idx, 1));
      CHECK(q.x == uv(tr.v2_idx, 0) && q.y == uv(tr.v2_idx, 1) && q.z == 0.0f && q.w == 0.0f);
    }
  }
  for (size_t s = 0; s < used.size(); ++s)
    if (!used[s]) CHECK(Zero(img.tris[3 * s]) && Zero(img.tris[3 * s + 1]) && Zero(img.tris[3 * s + 2]));
  // material records: one more than n_mats, the extra one zero but for the roughness of a zero exponent
  CHECK(img.mats.size() == 2 * ((size_t)n_mats + 1));
  bool sampled = false;
  for (uint32_t m = 0; m <= n_mats; ++m) {
    srt_material_obj o{};
    if (m < n_mats) o = c.mats[m];
    const float4 a = img.mats[2 * (size_t)m], b = img.mats[2 * (size_t)m + 1];
    CHECK(a.w == 1.0f / (o.specular_ex + 0.0000001f));
    CHECK(b.x == o.specular[0] && b.y == o.specular[1] && b.z == o.specular[2]);
    if (o.use_texture && c.albedo.empty()) {
      sampled = true;
      CHECK(a.x == 0.0f && a.y == 0.0f && a.z == 0.0f && U32(b.w) == o.handle[0] + 1);
    } else {
      const float* alb = o.use_texture ? &c.albedo[3 * (size_t)m] : o.diffuse;
      CHECK(a.x == alb[0] && a.y == alb[1] && a.z == alb[2] && U32(b.w) == 0);
    }
  }
  CHECK(img.sampled == sampled);
  CHECK(Zero(img.mats[2 * (size_t)n_mats + 1]) && img.mats[2 * (size_t)n_mats].x == 0.0f && img.mats[2 * (size_t)n_mats].z == 0.0f);
  // treelets: the flagged copy differs only in references; every path deeper than td passes exactly one
  // root; no right-spine flag steps onto one
  const int td = policy.treelet_depth;
  CHECK(img.nodes_t.empty() == img.troot.empty() && (img.nodes_t.empty() || img.nodes_t.size() == img.nodes.size()));
  CHECK(!img.nodes_t.empty() || !policy.treelets || img.depth <= td);
  if (img.nodes_t.empty()) return;
  const std::vector<float4>& hf = img.nodes_t;
  auto is_root = [&](uint32_t s) { return U32(hf[2 * (size_t)s + 3].w) == k.treelet_cnt; };
  struct Item { uint32_t s; int d, roots; };
  std::vector<Item> walk{{0u, 0, 0}};
  for (const auto& r : img.bvhs) walk.push_back({r.first_index, 0, 0});
  std::set<uint32_t> ids;
  while (!walk.empty()) {
    Item it = walk.back();
    walk.pop_back();
    uint32_t first = U32(hf[2 * (size_t)it.s + 2].w);
    if (is_root(it.s)) {
      CHECK(first < img.troot.size() && U32(img.nodes[2 * (size_t)it.s + 3].w) == 0);
      if (first >= img.troot.size()) return;
      ids.insert(first);
      ++it.roots;
      first = img.troot[first];
      CHECK(first == U32(img.nodes[2 * (size_t)it.s + 2].w));
    } else if (U32(hf[2 * (size_t)it.s + 3].w) != 0) {  // a leaf: the path ends
      CHECK(it.d > td ? it.roots == 1 : it.roots <= 1);
      continue;
    }
    walk.push_back({first | ror, it.d + 1, it.roots});
    walk.push_back({(first | ror) + 1, it.d + 1, it.roots});
  }
  CHECK(ids.size() == img.troot.size());
  for (uint32_t s = 0; s < img.n_slots; ++s) {
    const uint32_t first = U32(hf[2 * (size_t)s + 2].w);
    CHECK(std::memcmp(&hf[2 * (size_t)s + 2], &img.nodes[2 * (size_t)s + 2], 12) == 0);
    CHECK(std::memcmp(&hf[2 * (size_t)s + 3], &img.nodes[2 * (size_t)s + 3], 12) == 0);
    if (!ror || is_root(s) || U32(hf[2 * (size_t)s + 3].w) != 0 || !slots.count(s) || (first & 1u)) continue;
    CHECK(first + 2 < img.n_slots && !is_root(first + 2));
  }
}

static int g_pinned = 0;
static void RunCase(const Case& base) {
  for (const Config& g : Configs()) {
    const Case c = Apply(base, g);
    g_case = Tag(base, g);
    const srt::ScenePolicy policy =
        srt::ChooseScenePolicy((uint32_t)c.nodes.size(), (uint32_t)c.tris.size(), c.treelet_depth, 1);
    CHECK(policy.layout && policy.align == (g.align != 0) && policy.tri_align == (g.tri != 0) && policy.fused);
    CHECK(policy.top_depth == (g.pad ? g.top : 0) && policy.top_forced && policy.treelets && policy.global_waves == 5);
    srt::SceneImage img;
    std::vector<uint8_t> reach;
    std::vector<std::pair<uint32_t, uint32_t>> ranges;
    CHECK(Build(c, policy, kProduct, &img, &reach, &ranges) == SRT_OK);
    // (two records sharing a pair: the layout keeps the first placement and there is no top region)
    const bool top = g.pad && g.top && base.bvhs.size() == 1;
    CHECK(img.lds_ok && img.fused && (top ? img.top_depth > 0 && img.top_depth <= 3 : img.top_depth == 0));
    CheckImage(c, policy, img, reach, ranges);
    const unsigned long long fp[6] = {FnvOf(img.nodes), FnvOf(img.nodes_t), FnvOf(img.troot),
                                      FnvOf(img.mats),  FnvOf(img.tris),    FnvOf(img.tri_uv)};
    bool found = false;
    for (const Parent& p : kParent) {
      if (g_case != p.tag) continue;
      found = true;
      ++g_pinned;
      for (int a = 0; a < 6; ++a) CHECK(fp[a] == p.fp[a]);
    }
    CHECK(found);
  }
}

// Scalars at their edges, with small arrays.
static void TestScalars() {
  g_case = "scalars";
  for (const char* v : {"SRT_NODE_ALIGN", "SRT_TRI_ALIGN", "SRT_TOP_DEPTH", "SRT_GLOBAL_FUSED_MODE"}) unsetenv(v);
  // lds_ok flips at a 256-triangle leaf
  for (uint32_t big : {255u, 256u}) {
    Case c;
    c.nodes = {Node(0, 1, 0), Node(1, 0, big), Node(2, big, 1)};
    c.bvhs = {Record(0)};
    Geometry(&c, big + 1, true);
    srt::SceneImage img;
    std::vector<uint8_t> reach;
    std::vector<std::pair<uint32_t, uint32_t>> ranges;
    const srt::ScenePolicy policy = srt::ChooseScenePolicy(3, big + 1, 0, -1);
    CHECK(Build(c, policy, kProduct, &img, &reach, &ranges) == SRT_OK && img.lds_ok == (big == 255u));
    CHECK(img.nodes_t.empty() && img.depth == 1);
    CheckImage(c, policy, img, reach, ranges);
  }
  static_assert(srt::PackedEntries((1u << 24) - 1, (1u << 24) - 3, 255, kProduct), "");
  static_assert(!srt::PackedEntries(1u << 24, 8, 1, kProduct) && !srt::PackedEntries(8, (1u << 24) - 2, 1, kProduct) &&
                    !srt::PackedEntries(8, 8, 256, kProduct), "");
  // fused clears when an array passes 2^kCoopIdxBits float4 and COOP is on: the predicate at 29 bits, then
  // the image with 5 bits (32 float4: t7's 2 x (7 + 2 + 1) + 8 = 28 node float4 and 3 x (6 + 3) = 27 triangle
  // float4 fit, t15's 2 x (15 + 2 + 1) + 8 = 44 node float4 do not)
  srt::BuildConsts coop = kProduct;
  coop.coop = true;
  CHECK(srt::CoopIndexFits((1u << 28) - 6, 8, coop) && !srt::CoopIndexFits((1u << 28) - 5, 8, coop));
  CHECK(srt::CoopIndexFits(8, 178956967, coop) && !srt::CoopIndexFits(8, 178956968, coop));  // 3 x (n + 3) < 2^29
  coop.coop_idx_bits = 5;
  const std::vector<Case> cases = HandMadeCases();
  for (int which : {1, 3}) {
    srt::SceneImage img;
    std::vector<uint8_t> reach;
    std::vector<std::pair<uint32_t, uint32_t>> ranges;
    const Case& c = cases[(size_t)which];
    const srt::ScenePolicy policy = srt::ChooseScenePolicy((uint32_t)c.nodes.size(), (uint32_t)c.tris.size(), 0, -1);
    CHECK(policy.fused && !policy.align && !policy.tri_align && policy.top_depth == 0 && !policy.treelets);
    CHECK(Build(c, policy, coop, &img, &reach, &ranges) == SRT_OK && img.fused == (which == 1));
    CHECK(Build(c, policy, kProduct, &img, &reach, &ranges) == SRT_OK && img.fused);  // (no COOP: no limit)
  }
  // the policy's thresholds, in MB of 32-B nodes + 48-B triangles: 1 (triangle slots, top region), 48
  // (5 waves below), 192 (line-aligned chains from), 600 (fused below)
  const uint32_t mb = 1u << 15;  // nodes per MB
  srt::ScenePolicy p = srt::ChooseScenePolicy(mb - 1, 0, 0, -1);
  CHECK(!p.tri_align && p.top_depth == 0 && p.global_waves == 5 && !p.align && p.fused && !p.top_forced && p.layout);
  p = srt::ChooseScenePolicy(mb, 0, 0, -1);
  CHECK(p.tri_align && p.top_depth == 12 && p.treelet_depth == 1 && !p.treelets && !p.tl_scene);
  CHECK(srt::ChooseScenePolicy(48 * mb - 1, 0, 0, -1).global_waves == 5 && srt::ChooseScenePolicy(48 * mb, 0, 0, -1).global_waves == 4);
  CHECK(!srt::ChooseScenePolicy(192 * mb - 1, 0, 0, -1).align && srt::ChooseScenePolicy(192 * mb, 0, 0, -1).align);
  CHECK(srt::ChooseScenePolicy(600 * mb - 1, 0, 0, -1).fused);
  p = srt::ChooseScenePolicy(600 * mb, 0, 0, 1);
  CHECK(!p.fused && p.top_depth == 0 && p.treelets && p.treelet_depth == 9);  // 600 / 2^10 < 1 <= 600 / 2^9
  CHECK(srt::ChooseScenePolicy(mb, 0, 5, 0).treelet_depth == 5 && !srt::ChooseScenePolicy(mb, 0, 5, 0).treelets);
  setenv("SRT_NODE_LAYOUT", "0", 1);
  CHECK(!srt::ChooseScenePolicy(mb, 0, 0, -1).layout);
  unsetenv("SRT_NODE_LAYOUT");
}

static void TestRubik(const char* obj) {
  std::string err;
  const auto model = srt::LoadObjectFile(obj, false, &err);
  CHECK(model != nullptr);
  if (!model) return;
  const auto scene = srt::FlattenModels({model.get()}, &err);
  CHECK(scene != nullptr);
  if (!scene) return;
  Case c;
  c.name = "rubik";
  c.nodes = scene->nodes;
  c.bvhs = scene->bvhs;
  c.mats = scene->mats;
  c.albedo = scene->tex_albedo;
  c.tris = scene->tris;
  c.verts = scene->verts;
  c.treelet_depth = 3;
  RunCase(c);
  std::printf("Rubik: %zu triangles, %zu nodes\n", c.tris.size(), c.nodes.size());
}

int main(int argc, char** argv) {
  for (const Case& c : HandMadeCases()) RunCase(c);
  if (argc > 1) TestRubik(argv[1]);
  TestScalars();
  if (g_fail) {
    std::fprintf(stderr, "%d check(s) failed\n", g_fail);
    return 1;
  }
  std::printf("scene image checks OK (%d images pinned)\n", g_pinned);
  return 0;
}
