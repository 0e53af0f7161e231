// loudness_host_check.cpp — the host half of the loudness meter (bv2_api.cpp: bv2_loudness_plan / _coeffs / _blocks / _workspace_bytes and
// every argument check of bv2_loudness_measure / _gate / _apply) driven through the C API by a program of its own, so that it can run under
// host sanitizers without anything being loaded into Python and without a GPU:
//
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -x hip -Xarch_host -fsanitize=address,undefined -Iinclude \
//         tools/probe/loudness_host_check.cpp bert-vits2_amd/csrc/bv2_api.cpp -Wl,--unresolved-symbols=ignore-all -o /tmp/loudness_host_check
//   /tmp/loudness_host_check
//
// (The launchers and executors bv2_api.cpp names stay unresolved and are never reached: every call below either is a host function or is
// refused before its launch.  A call that got past its checks would jump to address 0 — which is what this program is there to show.)
// It checks the coefficients at 48 kHz against the table of ITU-R BS.1770-4, the plan and the block counts at the audio rates and at the
// edges of the envelope, the workspace size against the layout it must hold, and that each bad argument is refused with its code and a
// message that names it.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>

#include "../../include/bv2.h"

static int fails = 0;
static void expect(bool ok, const char* what) {
  if (ok) return;
  std::printf("FAIL: %s (last error: %s)\n", what, bv2_last_error(nullptr));
  ++fails;
}
static bool says(const char* word) { return std::strstr(bv2_last_error(nullptr), word) != nullptr; }

static bv2_loudness_config cfg_of(int rate, int fmt = BV2_WAV_F32) {
  bv2_loudness_config c;
  c.struct_bytes = (int32_t)sizeof(c);
  c.sample_rate = rate;
  c.input_format = fmt;
  return c;
}

int main() {
  // the standard's table (48 kHz): b0 b1 b2 a1 a2 of the shelf, a1 a2 of the high pass
  {
    const double want[7] = {1.53512485958697, -2.69169618940638, 1.19839281085285, -1.69065929318241, 0.73248077421585,
                            -1.99004745483398, 0.99007225036621};
    double c[10];
    bv2_loudness_config k = cfg_of(48000);
    expect(bv2_loudness_coeffs(&k, c) == 0, "coeffs at 48 kHz");
    double worst = 0;
    for (int i = 0; i < 5; ++i) worst = std::fmax(worst, std::fabs(c[i] - want[i]));
    worst = std::fmax(worst, std::fmax(std::fabs(c[8] - want[5]), std::fabs(c[9] - want[6])));
    std::printf("48 kHz: max |coeff - table| = %.3e\n", worst);
    expect(worst <= 1e-12 && c[5] == 1.0 && c[6] == -2.0 && c[7] == 1.0, "the table of BS.1770-4");
  }
  for (int rate : {8000, 16000, 22050, 24000, 44100, 48000, 96000, 192000}) {
    bv2_loudness_config k = cfg_of(rate);
    int32_t step = 0, block = 0, tile = 0;
    expect(bv2_loudness_plan(&k, &step, &block, &tile) == 0, "plan");
    expect(step == (int)std::floor(rate / 10.0 + 0.5) && block == 4 * step && tile > 0 && (tile - 1) / step + 2 <= 8, "step, block, tile");
    expect(bv2_loudness_plan(&k, nullptr, nullptr, nullptr) == 0, "plan with null outputs");
    const int64_t n[7] = {0, 1, block - 1, block, block + step - 1, block + step, 10 * (int64_t)block + 3};
    const int64_t want[7] = {0, 1, 1, 1, 1, 2, 37};
    for (int i = 0; i < 7; ++i) expect(bv2_loudness_blocks(&k, n[i]) == want[i], "block count");
    expect(bv2_loudness_blocks(&k, -1) < 0 && says("n must be"), "negative n refused");
    double c[10];
    expect(bv2_loudness_coeffs(&k, c) == 0 && c[0] > 1.0 && c[3] < 0 && c[4] > 0 && c[4] < 1 && c[9] > 0 && c[9] < 1, "coeffs are a stable pair");
    // the workspace holds 16 tile states, partial sums and a peak per tile, 32 bytes per item and the block table
    const int32_t B = 3;
    const int64_t S = 5 * (int64_t)tile + 17, nt = 6;
    const int64_t floor_bytes = B * nt * (4 * 8 + 4 * 8 + 8 * 8 + 4) + B * 32 + B * bv2_loudness_blocks(&k, S) * 8;
    expect(bv2_loudness_workspace_bytes(&k, B, S) >= floor_bytes, "workspace size");
  }

  void* p = reinterpret_cast<void*>(4096);                     // never followed: every call below is refused first
  double* pd = static_cast<double*>(p);
  float* pf = static_cast<float*>(p);
  int32_t* pi = static_cast<int32_t*>(p);
  int16_t* ps = static_cast<int16_t*>(p);
  bv2_loudness_config good = cfg_of(44100), low = cfg_of(7999), high = cfg_of(192001), fmt = cfg_of(44100, 9), drift = cfg_of(44100);
  drift.struct_bytes = 8;
  int32_t v = 0;
  double c[10];
  for (bv2_loudness_config* k : {&low, &high, &fmt, &drift}) {
    const char* word = k == &fmt ? "input_format" : (k == &drift ? "struct_bytes" : "sample_rate");
    expect(bv2_loudness_plan(k, &v, &v, &v) == -1 && says(word), "plan refuses a bad config");
    expect(bv2_loudness_coeffs(k, c) == -1 && says(word), "coeffs refuses a bad config");
    expect(bv2_loudness_blocks(k, 5) < 0 && bv2_loudness_workspace_bytes(k, 1, 5) < 0, "the size queries refuse a bad config");
    expect(bv2_loudness_measure(nullptr, k, p, 10, nullptr, 1, 10, nullptr, 1, -23, -1, pd, pf, pf, pi, nullptr, p, 1 << 20) == -1 && says(word),
           "measure refuses a bad config");
    expect(bv2_loudness_gate(nullptr, k, pd, 1, nullptr, 1, 10, pf, nullptr, 1, -23, -1, pd, pf, pi, p, 1 << 20) == -1 && says(word),
           "gate refuses a bad config");
    expect(bv2_loudness_apply(nullptr, k, p, 10, nullptr, 1, 10, nullptr, 1, pf, pf, nullptr, 10) == -1 && says(word), "apply refuses a bad config");
  }
  expect(bv2_loudness_plan(nullptr, &v, &v, &v) == -1 && says("cfg is null"), "null cfg");
  expect(bv2_loudness_coeffs(&good, nullptr) == -1 && says("out is null"), "null out");
  expect(bv2_loudness_workspace_bytes(&good, 0, 10) < 0 && bv2_loudness_workspace_bytes(&good, 4097, 10) < 0 &&
         bv2_loudness_workspace_bytes(&good, 1, 0) < 0 && bv2_loudness_workspace_bytes(&good, 1, (int64_t)1 << 31) < 0, "workspace query envelope");

  const int64_t S = 10000, need = bv2_loudness_workspace_bytes(&good, 2, S);
  const double nan = std::nan("");
  auto measure = [&](const void* wav, int32_t B, int64_t S_, const int32_t* groups, int32_t ng, double target, double* lufs, float* gain,
                     float* peak, int32_t* flags, double* ms, void* ws, int64_t bytes, int64_t stride) {
    return bv2_loudness_measure(nullptr, &good, wav, stride, nullptr, B, S_, groups, ng, target, -1.0, lufs, gain, peak, flags, ms, ws, bytes);
  };
  expect(measure(nullptr, 2, S, nullptr, 2, -23, pd, pf, pf, pi, nullptr, p, need, S) == -1 && says("wav is null"), "measure: null wav");
  expect(measure(p, 2, S, nullptr, 2, -23, pd, pf, nullptr, pi, nullptr, p, need, S) == -1 && says("peak is null"), "measure: null peak");
  expect(measure(p, 2, S, nullptr, 2, -23, nullptr, pf, pf, pi, nullptr, p, need, S) == -1 && says("go together"), "measure: lufs alone missing");
  expect(measure(p, 2, S, nullptr, 2, -23, nullptr, nullptr, pf, nullptr, nullptr, p, need, S) == -1 && says("block_ms is null"), "measure: nothing to produce");
  expect(measure(p, 0, S, nullptr, 0, -23, pd, pf, pf, pi, nullptr, p, need, S) == -1 && says("B must be"), "measure: B < 1");
  expect(measure(p, 4097, S, nullptr, 4097, -23, pd, pf, pf, pi, nullptr, p, need, S) == -1 && says("B must be"), "measure: B too large");
  expect(measure(p, 2, 0, nullptr, 2, -23, pd, pf, pf, pi, nullptr, p, need, S) == -1 && says("S must be"), "measure: S < 1");
  expect(measure(p, 2, S, nullptr, 1, -23, pd, pf, pf, pi, nullptr, p, need, S) == -1 && says("n_groups"), "measure: n_groups without groups");
  expect(measure(p, 2, S, pi, 3, -23, pd, pf, pf, pi, nullptr, p, need, S) == -1 && says("n_groups"), "measure: n_groups > B");
  expect(measure(p, 2, S, pi, 0, -23, pd, pf, pf, pi, nullptr, p, need, S) == -1 && says("n_groups"), "measure: n_groups < 1");
  expect(measure(p, 2, S, nullptr, 2, nan, pd, pf, pf, pi, nullptr, p, need, S) == -1 && says("finite"), "measure: NaN target");
  expect(measure(p, 2, S, nullptr, 2, -23, pd, pf, pf, pi, nullptr, p, need, -1) == -1 && says("wav_bstride"), "measure: negative stride");
  expect(measure(p, 2, S, nullptr, 2, -23, pd, pf, pf, pi, nullptr, nullptr, need, S) == -5 && says("workspace"), "measure: null workspace");
  expect(measure(p, 2, S, nullptr, 2, -23, pd, pf, pf, pi, nullptr, p, need - 257, S) == -5 && says("workspace"), "measure: short workspace");
  expect(measure(reinterpret_cast<void*>(4097), 2, S, nullptr, 2, -23, pd, pf, pf, pi, nullptr, reinterpret_cast<void*>(4097), need - 256, S) == -5,
         "measure: a misaligned workspace needs its slack");

  auto gate = [&](const double* ms, int64_t stride, int32_t B, int64_t S_, const float* peak, const int32_t* groups, int32_t ng, double* lufs,
                  void* ws, int64_t bytes) {
    return bv2_loudness_gate(nullptr, &good, ms, stride, nullptr, B, S_, peak, groups, ng, -23.0, -1.0, lufs, pf, pi, ws, bytes);
  };
  expect(gate(nullptr, 4, 2, S, pf, nullptr, 2, pd, p, 1024) == -1 && says("must not be null"), "gate: null block_ms");
  expect(gate(pd, 4, 2, S, nullptr, nullptr, 2, pd, p, 1024) == -1 && says("must not be null"), "gate: null peak");
  expect(gate(pd, 4, 2, S, pf, nullptr, 2, nullptr, p, 1024) == -1 && says("must not be null"), "gate: null lufs");
  expect(gate(pd, 4, 0, S, pf, nullptr, 0, pd, p, 1024) == -1 && says("B must be"), "gate: B < 1");
  expect(gate(pd, 4, 2, S, pf, nullptr, 3, pd, p, 1024) == -1 && says("n_groups"), "gate: n_groups");
  expect(gate(pd, 4, 2, S, pf, nullptr, 2, pd, nullptr, 1024) == -5 && says("workspace"), "gate: null workspace");
  expect(gate(pd, 4, 2, S, pf, nullptr, 2, pd, p, 63) == -5 && says("workspace"), "gate: short workspace");
  expect(gate(pd, 3, 2, 4 * 17640, pf, nullptr, 2, pd, p, 1024) == -1 && says("ms_bstride"), "gate: short rows");

  auto apply = [&](const void* src, int64_t ss, int32_t B, int64_t S_, const int32_t* groups, int32_t ng, const float* gain, float* f32,
                   int16_t* i16, int64_t ds) {
    return bv2_loudness_apply(nullptr, &good, src, ss, nullptr, B, S_, groups, ng, gain, f32, i16, ds);
  };
  expect(apply(nullptr, S, 2, S, nullptr, 2, pf, pf, nullptr, S) == -1 && says("src is null"), "apply: null src");
  expect(apply(p, S, 2, S, nullptr, 2, nullptr, pf, nullptr, S) == -1 && says("gain is null"), "apply: null gain");
  expect(apply(p, S, 2, S, nullptr, 2, pf, pf, ps, S) == -1 && says("exactly one"), "apply: both destinations");
  expect(apply(p, S, 2, S, nullptr, 2, pf, nullptr, nullptr, S) == -1 && says("exactly one"), "apply: no destination");
  expect(apply(p, S, 0, S, nullptr, 0, pf, pf, nullptr, S) == -1 && says("B must be"), "apply: B < 1");
  expect(apply(p, S, 2, 0, nullptr, 2, pf, pf, nullptr, S) == -1 && says("S must be"), "apply: S < 1");
  expect(apply(p, S, 2, S, nullptr, 1, pf, pf, nullptr, S) == -1 && says("n_groups"), "apply: n_groups without groups");
  expect(apply(p, S, 2, S, pi, 0, pf, pf, nullptr, S) == -1 && says("n_groups"), "apply: an empty gain table");
  expect(apply(p, S, 65536, S, nullptr, 65536, pf, pf, nullptr, S) == -1 && says("B must be"), "apply: B too large");
  expect(apply(p, S, 2, S, nullptr, 2, pf, pf, nullptr, S - 1) == -1 && says("dst_bstride"), "apply: short destination rows");
  expect(apply(p, -1, 2, S, nullptr, 2, pf, pf, nullptr, S) == -1 && says("src_bstride"), "apply: negative source stride");

  std::printf(fails ? "%d check(s) failed\n" : "loudness_host_check: all checks passed\n", fails);
  return fails ? 1 : 0;
}
