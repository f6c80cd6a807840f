// The host-only parts of include/srt_variance.h (csrc/temporal_host.cpp, csrc/denoise_host.cpp) as a stand-alone
// program, meant for AddressSanitizer + UBSan on the CPU (no device, no HIP):
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude
//       tests/cpp/test_variance_host.cpp simple-ray-tracer_amd/csrc/temporal_host.cpp
//       simple-ray-tracer_amd/csrc/denoise_host.cpp -o test_variance_host
// It checks the validation of srt_denoise_var_params, the sizing of the moment and variance arrays, the state of
// the moment history under mixed accumulate calls and the launch schedule of the variance-guided filter.
#include <cstdio>
#include <limits>

#include "../../simple-ray-tracer_amd/csrc/denoise_host.hpp"
#include "../../simple-ray-tracer_amd/csrc/temporal_host.hpp"

static int g_fail = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
      ++g_fail;                                                            \
    }                                                                      \
  } while (0)

static void TestVarParams() {
  using namespace srt::denoise;
  const srt_denoise_var_params d = DefaultVarParams();
  CHECK(d.sigma_lum == 1.0f && d.min_history == 4);
  CHECK(ValidateVarParams(&d) == SRT_OK);
  CHECK(ValidateVarParams(nullptr) == SRT_ERR_INVALID);
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  const float bad[] = {0.0f, -0.0f, -1.0f, inf, -inf, nan};
  for (float b : bad) {
    srt_denoise_var_params p = d;
    p.sigma_lum = b;
    CHECK(ValidateVarParams(&p) == SRT_ERR_INVALID);
  }
  srt_denoise_var_params p = d;
  p.sigma_lum = std::numeric_limits<float>::denorm_min();
  p.min_history = 1;
  CHECK(ValidateVarParams(&p) == SRT_OK);
  p.sigma_lum = std::numeric_limits<float>::max();
  p.min_history = 65535;
  CHECK(ValidateVarParams(&p) == SRT_OK);
  const uint32_t bad_h[] = {0u, 65536u, 0xFFFFFFFFu};
  for (uint32_t b : bad_h) {
    p = d;
    p.min_history = b;
    CHECK(ValidateVarParams(&p) == SRT_ERR_INVALID);
  }
}

static void TestSizes() {
  srt::temporal::Sizes ts;
  CHECK(srt::temporal::PlanBuffers(70, 41, &ts) == SRT_OK);
  CHECK(srt::temporal::MomentBytes(ts) == 8u * 70 * 41 && ts.scratch_bytes == 72u * 70 * 41);  // two arrays: 16 B a pixel
  CHECK(srt::temporal::PlanBuffers(16384, 16384, &ts) == SRT_OK && srt::temporal::MomentBytes(ts) == (size_t)1 << 31);
  srt::denoise::Sizes ds;
  CHECK(srt::denoise::PlanBuffers(70, 41, &ds) == SRT_OK);
  CHECK(srt::denoise::VarianceBytes(ds) == 4u * 70 * 41 && ds.scratch_bytes == 48u * 70 * 41);  // two arrays: 8 B a pixel
  CHECK(srt::denoise::PlanBuffers(1, 1, &ds) == SRT_OK && srt::denoise::VarianceBytes(ds) == 4);
}

static void TestMomentState() {
  using namespace srt::temporal;
  History h;
  Moments m;
  const srt_temporal_camera c = {{1, 2, 3}, {0, 0, -1}, {1, 0, 0}, {0, 1, 0}};
  CHECK(!m.enabled && !m.valid && MomentsHavePrev(m, h) == 0);
  AdvanceMoments(&m, true);  // not enabled: nothing becomes valid
  CHECK(!m.valid);
  Advance(&h, c);            // a plain frame before moments are enabled
  EnableMoments(&m);
  CHECK(m.enabled && !m.valid && MomentsHavePrev(m, h) == 0);  // a colour history, but no moments of that frame
  Advance(&h, c);
  AdvanceMoments(&m, true);
  CHECK(m.valid && MomentsHavePrev(m, h) == 1);
  EnableMoments(&m);  // idempotent: the history stays
  CHECK(m.enabled && m.valid);
  Advance(&h, c);
  AdvanceMoments(&m, false);  // a plain call in between
  CHECK(h.valid && !m.valid && MomentsHavePrev(m, h) == 0);
  Advance(&h, c);
  AdvanceMoments(&m, true);
  CHECK(MomentsHavePrev(m, h) == 1);
  const int wrote = WriteIndex(h);
  Advance(&h, c);
  AdvanceMoments(&m, true);
  CHECK(h.read == wrote);  // the moments ride on the colour history's set indices
  Reset(&h);
  ResetMoments(&m);
  CHECK(m.enabled && !m.valid && MomentsHavePrev(m, h) == 0);
  Advance(&h, c);
  AdvanceMoments(&m, true);
  CHECK(MomentsHavePrev(m, h) == 1);
  Reset(&h);  // the colour history alone gone: still nothing to read
  CHECK(MomentsHavePrev(m, h) == 0);
}

static void TestSchedule() {
  using namespace srt::denoise;
  srt_denoise_params p = DefaultParams();
  VarLaunch s[SRT_DENOISE_MAX_PASSES + 1];
  CHECK(BuildVarianceSchedule(p, 70, 41, s) == 6);
  CHECK(s[0].resolve && !s[0].last && s[0].src == kAccum && s[0].dst == kPing && s[0].step == 0);
  for (int l = 1; l <= 5; ++l) {
    CHECK(!s[l].resolve && s[l].step == 1 << (l - 1) && s[l].src == s[l - 1].dst && s[l].last == (l == 5));
    CHECK(s[l].last ? s[l].dst == kOutput : (s[l].dst == (s[l].src ^ 1)));
    CHECK(s[l].grid_x == 2 && s[l].grid_y == 11);
  }
  p.passes = 1;
  CHECK(BuildVarianceSchedule(p, 1, 1, s) == 2 && s[1].last && s[1].src == kPing && s[1].dst == kOutput && s[1].grid_x == 1);
  p.passes = 8;
  CHECK(BuildVarianceSchedule(p, 65535, 4, s) == 9 && s[8].last && s[8].step == 128 && s[8].grid_x == 1024 && s[8].grid_y == 1);
  p.passes = 0;
  CHECK(BuildVarianceSchedule(p, 70, 41, s) == 0);
  p.passes = 1000;  // clamped as BuildSchedule clamps it; ValidateParams never lets it in
  CHECK(BuildVarianceSchedule(p, 70, 41, s) == 9);
}

int main() {
  TestVarParams();
  TestSizes();
  TestMomentState();
  TestSchedule();
  if (g_fail) {
    std::fprintf(stderr, "%d check(s) failed\n", g_fail);
    return 1;
  }
  std::printf("variance host checks OK\n");
  return 0;
}
