// r128_host_check.cpp — the host half of true peak, step energies and loudness range (bv2_api.cpp: bv2_true_peak_plan / _workspace_bytes,
// bv2_loudness_steps_count, bv2_loudness_range_workspace_bytes and every argument check of bv2_true_peak / bv2_loudness_steps /
// bv2_loudness_range) driven through the C API by a program of its own, so that it can run under host sanitizers without anything being
// loaded into Python and without a GPU (tools/probe/loudness_host_check.cpp is its elder; the same build line):
//
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -x hip -Xarch_host -fsanitize=address,undefined -Iinclude \
//         tools/probe/r128_host_check.cpp bert-vits2_amd/csrc/bv2_api.cpp -Wl,--unresolved-symbols=ignore-all -o /tmp/r128_host_check
//   /tmp/r128_host_check
//
// Every device call below is refused before its launch; a call that got past its checks would jump to address 0.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

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
  const int rates[7] = {8000, 44100, 48000, 95999, 96000, 191999, 192000};
  const int factors[7] = {4, 4, 4, 4, 2, 2, 1};
  for (int i = 0; i < 7; ++i) {
    bv2_loudness_config k = cfg_of(rates[i]);
    int32_t F = 0, K = -1;
    expect(bv2_true_peak_plan(&k, &F, &K) == 0 && F == factors[i] && K == (F > 1 ? 36 : 0), "true peak plan");
    expect(bv2_true_peak_plan(&k, nullptr, nullptr) == 0, "plan with null outputs");
    if (F > 1) {                                              // the table the kernel reads is the resampler's at rate -> F rate: F rows of 73
      bv2_resample_config r = {(int32_t)sizeof(bv2_resample_config), rates[i], F * rates[i], BV2_WAV_F32};
      int32_t L = 0, M = 0, K2 = 0;
      expect(bv2_resample_plan(&r, &L, &M, &K2) == 0 && L == F && M == 1 && K2 == 36, "the resampler's plan at rate -> F rate");
      std::vector<float> t((size_t)F * 73);
      expect(bv2_resample_taps(&r, t.data()) == 0 && t[36] > 0.90f && t[36] < 0.92f, "phase 0 has a centre tap of 0.91");
    }
    const int step = (rates[i] + 5) / 10;
    expect(bv2_loudness_steps_count(&k, 0) == 0 && bv2_loudness_steps_count(&k, step - 1) == 0 && bv2_loudness_steps_count(&k, step) == 1 &&
           bv2_loudness_steps_count(&k, 30 * (int64_t)step + 7) == 30, "whole steps");
    expect(bv2_loudness_steps_count(&k, -1) < 0 && says("n must be"), "negative n refused");
    const int64_t S = 5 * (int64_t)BV2_TRUE_PEAK_TILE + 17;
    expect(bv2_true_peak_workspace_bytes(&k, 3, S) >= 3 * 6 * 4, "one fp32 per tile");
    expect(bv2_loudness_range_workspace_bytes(&k, 3, S) >= 3 * (S / step > 0 ? S / step : 1) * 8, "one fp64 per step");
  }

  void* p = reinterpret_cast<void*>(4096);                     // never followed: every call below is refused first
  double* pd = static_cast<double*>(p);
  float* pf = static_cast<float*>(p);
  int32_t* pi = static_cast<int32_t*>(p);
  bv2_loudness_config good = cfg_of(44100), low = cfg_of(7999), high = cfg_of(192001), fmt = cfg_of(44100, 9), drift = cfg_of(44100);
  drift.struct_bytes = 8;
  const int64_t S = 100000;
  for (bv2_loudness_config* k : {&low, &high, &fmt, &drift}) {
    const char* word = k == &fmt ? "input_format" : (k == &drift ? "struct_bytes" : "sample_rate");
    int32_t v = 0;
    expect(bv2_true_peak_plan(k, &v, &v) == -1 && says(word), "plan refuses a bad config");
    expect(bv2_true_peak_workspace_bytes(k, 1, S) < 0 && bv2_loudness_range_workspace_bytes(k, 1, S) < 0 && bv2_loudness_steps_count(k, 5) < 0,
           "the size queries refuse a bad config");
    expect(bv2_true_peak(nullptr, k, pf, p, S, nullptr, 1, S, pf, p, 1 << 20) == -1 && says(word), "true_peak refuses a bad config");
    expect(bv2_loudness_steps(nullptr, k, p, S, nullptr, 1, S, pd, 30, nullptr, nullptr, p, 1 << 24) == -1 && says(word), "steps refuses a bad config");
    expect(bv2_loudness_range(nullptr, k, pd, 30, nullptr, 1, S, nullptr, 1, pd, pd, pd, pd, pd, pi, p, 1 << 20) == -1 && says(word),
           "range refuses a bad config");
  }
  expect(bv2_true_peak_plan(nullptr, nullptr, nullptr) == -1 && says("cfg is null"), "null cfg");
  expect(bv2_true_peak_workspace_bytes(&good, 0, S) < 0 && bv2_true_peak_workspace_bytes(&good, 4097, S) < 0 &&
         bv2_true_peak_workspace_bytes(&good, 1, 0) < 0 && bv2_true_peak_workspace_bytes(&good, 1, (int64_t)1 << 31) < 0, "true peak workspace envelope");
  expect(bv2_loudness_range_workspace_bytes(&good, 0, S) < 0 && bv2_loudness_range_workspace_bytes(&good, 1, 0) < 0, "range workspace envelope");

  int64_t need = bv2_true_peak_workspace_bytes(&good, 2, S);
  auto tp = [&](const float* taps, const void* wav, int64_t stride, int32_t B, int64_t S_, float* out, void* ws, int64_t bytes) {
    return bv2_true_peak(nullptr, &good, taps, wav, stride, nullptr, B, S_, out, ws, bytes);
  };
  expect(tp(pf, nullptr, S, 2, S, pf, p, need) == -1 && says("wav is null"), "true_peak: null wav");
  expect(tp(pf, p, S, 2, S, nullptr, p, need) == -1 && says("peak_out is null"), "true_peak: null output");
  expect(tp(nullptr, p, S, 2, S, pf, p, need) == -1 && says("taps is null"), "true_peak: null taps at F = 4");
  expect(tp(pf, p, -1, 2, S, pf, p, need) == -1 && says("wav_bstride"), "true_peak: negative stride");
  expect(tp(pf, p, S, 0, S, pf, p, need) == -1 && says("B must be"), "true_peak: B < 1");
  expect(tp(pf, p, S, 4097, S, pf, p, need) == -1 && says("B must be"), "true_peak: B too large");
  expect(tp(pf, p, S, 2, 0, pf, p, need) == -1 && says("S must be"), "true_peak: S < 1");
  expect(tp(pf, p, S, 2, S, pf, nullptr, need) == -5 && says("workspace"), "true_peak: null workspace");
  expect(tp(pf, p, S, 2, S, pf, p, need - 257) == -5 && says("workspace"), "true_peak: short workspace");
  expect(tp(pf, p, S, 2, S, pf, reinterpret_cast<void*>(4097), need - 256) == -5, "true_peak: a misaligned workspace needs its slack");

  need = bv2_loudness_workspace_bytes(&good, 2, S);
  auto steps = [&](const void* wav, int64_t stride, int32_t B, int64_t S_, double* ss, int64_t ss_stride, void* ws, int64_t bytes) {
    return bv2_loudness_steps(nullptr, &good, wav, stride, nullptr, B, S_, ss, ss_stride, nullptr, nullptr, ws, bytes);
  };
  expect(steps(nullptr, S, 2, S, pd, 22, p, need) == -1 && says("wav is null"), "steps: null wav");
  expect(steps(p, S, 2, S, nullptr, 22, p, need) == -1 && says("step_ss is null"), "steps: null step_ss");
  expect(steps(p, -1, 2, S, pd, 22, p, need) == -1 && says("wav_bstride"), "steps: negative stride");
  expect(steps(p, S, 0, S, pd, 22, p, need) == -1 && says("B must be"), "steps: B < 1");
  expect(steps(p, S, 2, 0, pd, 22, p, need) == -1 && says("S must be"), "steps: S < 1");
  expect(steps(p, S, 2, S, pd, 21, p, need) == -1 && says("ss_bstride"), "steps: short rows");
  expect(steps(p, S, 2, S, pd, 22, nullptr, need) == -5 && says("workspace"), "steps: null workspace");
  expect(steps(p, S, 2, S, pd, 22, p, need - 257) == -5 && says("workspace"), "steps: short workspace");

  need = bv2_loudness_range_workspace_bytes(&good, 2, S);
  auto range = [&](const double* ss, int64_t ss_stride, int32_t B, int64_t S_, const int32_t* groups, int32_t ng, double* lra, int32_t* flags,
                   void* ws, int64_t bytes) {
    return bv2_loudness_range(nullptr, &good, ss, ss_stride, nullptr, B, S_, groups, ng, lra, pd, pd, pd, pd, flags, ws, bytes);
  };
  expect(range(nullptr, 22, 2, S, nullptr, 2, pd, pi, p, need) == -1 && says("must not be null"), "range: null step_ss");
  expect(range(pd, 22, 2, S, nullptr, 2, nullptr, pi, p, need) == -1 && says("must not be null"), "range: null lra");
  expect(range(pd, 22, 2, S, nullptr, 2, pd, nullptr, p, need) == -1 && says("must not be null"), "range: null flags");
  expect(range(pd, 22, 0, S, nullptr, 0, pd, pi, p, need) == -1 && says("B must be"), "range: B < 1");
  expect(range(pd, 22, 2, 0, nullptr, 2, pd, pi, p, need) == -1 && says("S must be"), "range: S < 1");
  expect(range(pd, 22, 2, S, nullptr, 1, pd, pi, p, need) == -1 && says("n_groups"), "range: n_groups without groups");
  expect(range(pd, 22, 2, S, pi, 3, pd, pi, p, need) == -1 && says("n_groups"), "range: n_groups > B");
  expect(range(pd, 21, 2, S, nullptr, 2, pd, pi, p, need) == -1 && says("ss_bstride"), "range: short rows");
  expect(range(pd, 22, 2, S, nullptr, 2, pd, pi, nullptr, need) == -5 && says("workspace"), "range: null workspace");
  expect(range(pd, 22, 2, S, nullptr, 2, pd, pi, p, need - 257) == -5 && says("workspace"), "range: short workspace");

  std::printf(fails ? "%d check(s) failed\n" : "r128_host_check: all checks passed\n", fails);
  return fails ? 1 : 0;
}
