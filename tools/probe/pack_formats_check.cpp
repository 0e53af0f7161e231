// pack_formats_check.cpp — the writers of the packed weight formats (bv2_pack.h) driven by a program of its own, so that they can run
// under host sanitizers without anything being loaded into Python and without a GPU:
//
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -x hip -Xarch_host -fsanitize=address,undefined -Iinclude \
//         tools/probe/pack_formats_check.cpp bert-vits2_amd/csrc/kernels/resblock_cl_bf16.hip -Wl,--unresolved-symbols=ignore-all \
//         -o /tmp/pack_formats_check
//   /tmp/pack_formats_check
//
// (resblock_cl_bf16.hip defines resblock_cl_bf16_units, the unit padding of the tap-major stream; nothing else of it is reached.)
// Every writer fills a zeroed host buffer of EXACTLY its format's element count — a write past it is the sanitizer's to find — from a dense
// weight of distinct non-zero values.  Reading back through the format's index function must return every (co, ci, j), and the non-zero
// elements must be exactly the indexed ones: every weight landed once, nothing was written beside them.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../bert-vits2_amd/csrc/bv2_pack.h"

using namespace bv2;

static int fails = 0;
static void expect(bool ok, const char* fmt, int a, int b, int c) {
  if (ok) return;
  std::printf("FAIL: ");
  std::printf(fmt, a, b, c);
  std::printf("\n");
  ++fails;
}

// distinct, non-zero, both signs, magnitudes over three decades (the x3 form scales by the largest)
static std::vector<float> dense(int cin, int cout, int k, int salt = 0) {
  std::vector<float> w((size_t)cout * cin * k);
  for (size_t i = 0; i < w.size(); ++i) w[i] = (float)(i + 1 + 7 * salt) * 3.7e-4f * ((i + salt) % 3 == 0 ? -1.f : 1.f);
  return w;
}
static float bf2f(uint16_t b) { const uint32_t u = (uint32_t)b << 16; float f; std::memcpy(&f, &u, 4); return f; }

// `named` marks the elements the index function names; returns true when the non-zero elements of `buf` are exactly inside them
template <class T>
static bool only_named(const std::vector<T>& buf, const std::vector<char>& named) {
  for (size_t i = 0; i < buf.size(); ++i)
    if (buf[i] != 0 && !named[i]) return false;
  return true;
}
template <class T>
static int64_t nonzero(const std::vector<T>& buf) {
  int64_t n = 0;
  for (const T& v : buf) n += v != 0;
  return n;
}

static void check_f32(int cin, int cout, int k) {
  const ConvW c = conv_desc(cin, cout, k);
  const std::vector<float> w = dense(cin, cout, k);
  std::vector<float> buf((size_t)c.cout_pad * c.cin_pad * k, 0.f);           // 32-row tiles x 8-channel groups, whole
  pack_f32(buf.data(), cin, cout, k, [&](int co, int ci, int j) { return w[((size_t)co * cin + ci) * k + j]; });
  bool back = true;
  for (int co = 0; co < cout; ++co)
    for (int ci = 0; ci < cin; ++ci)
      for (int j = 0; j < k; ++j) back = back && buf[(size_t)conv_w_index(j, ci, co, c.cin_pad, k)] == w[((size_t)co * cin + ci) * k + j];
  expect(back, "fp32 (%d, %d, %d): read back", cin, cout, k);
  expect(nonzero(buf) == (int64_t)cout * cin * k, "fp32 (%d, %d, %d): every element once", cin, cout, k);
  std::vector<float> brow((size_t)c.cout_pad, 0.f);
  pack_bias(brow.data(), cout, [&](int co) { return w[(size_t)co]; });
  bool bok = nonzero(brow) == cout;
  for (int co = 0; co < cout; ++co) bok = bok && brow[(size_t)co] == w[(size_t)co];
  expect(bok, "bias row (%d, %d, %d)", cin, cout, k);
}

static void check_cl(int cin, int cout, int k) {
  const ConvW c = conv_cl_desc(cin, cout, k);
  const std::vector<float> w = dense(cin, cout, k);
  const auto src = [&](int co, int ci, int j) { return w[((size_t)co * cin + ci) * k + j]; };
  const int64_t N = (int64_t)cout * cin * k;
  for (int f16 = 0; f16 < 2; ++f16) {
    std::vector<uint16_t> buf((size_t)cl_w_elems(cin, c.cout_pad, k), 0);
    if (f16) pack_cl_f16(buf.data(), cin, cout, k, src);
    else pack_cl_bf16(buf.data(), cin, cout, k, src);
    bool back = true;
    for (int co = 0; co < cout; ++co)
      for (int ci = 0; ci < cin; ++ci)
        for (int j = 0; j < k; ++j) back = back && buf[(size_t)cl_w_index(j, ci, co, cin, k)] == (f16 ? f2h(src(co, ci, j)) : f2bf(src(co, ci, j)));
    expect(back, f16 ? "fp16 channels-last (%d, %d, %d): read back" : "bf16 channels-last (%d, %d, %d): read back", cin, cout, k);
    expect(nonzero(buf) == N, "channels-last (%d, %d, %d): every element once", cin, cout, k);
  }
  {                                                                         // x6: w = h1 + h2 + h3 exactly
    std::vector<uint16_t> buf((size_t)x6_w_elems(cin, c.cout_pad, k), 0);
    std::vector<char> named(buf.size(), 0);
    pack_x6(buf.data(), cin, cout, k, src);
    bool back = true;
    int64_t first = 0;
    for (int co = 0; co < cout; ++co)
      for (int ci = 0; ci < cin; ++ci)
        for (int j = 0; j < k; ++j) {
          double sum = 0;
          for (int pl = 0; pl < 3; ++pl) {
            const size_t at = (size_t)x6_w_index(j, ci, co, cin, k, pl);
            back = back && !named[at];
            named[at] = 1;
            sum += (double)bf2f(buf[at]);
          }
          first += buf[(size_t)x6_w_index(j, ci, co, cin, k, 0)] != 0;
          back = back && sum == (double)src(co, ci, j);
        }
    expect(back, "x6 (%d, %d, %d): the three planes sum to w", cin, cout, k);
    expect(first == N && only_named(buf, named), "x6 (%d, %d, %d): every element once", cin, cout, k);
  }
  {                                                                         // x3: w * S_w = g0 + g1, |w * S_w| < 2^15
    std::vector<uint16_t> buf((size_t)x3_w_elems(cin, c.cout_pad, k), 0);
    std::vector<char> named(buf.size(), 0);
    const float inv = pack_x3(buf.data(), cin, cout, k, src);
    const float S = 1.f / inv;                                               // a power of two: exact
    bool back = true, range = true;
    int64_t first = 0;
    for (int co = 0; co < cout; ++co)
      for (int ci = 0; ci < cin; ++ci)
        for (int j = 0; j < k; ++j) {
          const size_t a0 = (size_t)x3_w_index(j, ci, co, cin, k, 0), a1 = (size_t)x3_w_index(j, ci, co, cin, k, 1);
          back = back && !named[a0] && !named[a1] && a0 != a1;
          named[a0] = named[a1] = 1;
          first += buf[a0] != 0;
          const double v = (double)src(co, ci, j) * S, got = (double)h2f(buf[a0]) + (double)h2f(buf[a1]);
          // one rounding of the pair: g1 keeps 11 bits of the remainder v - g0 (at most 2^-11 |v|), so 2^-23 |v|; where the remainder
          // falls into fp16's subnormals their spacing 2^-24 bounds it instead, half of it = 2^-25 (bv2_kernels.h, the x3 form)
          back = back && std::fabs(got - v) <= std::max(std::ldexp(std::fabs(v), -23), std::ldexp(1.0, -25));
          back = back && std::fabs(got * inv - (double)src(co, ci, j)) <= std::max(std::ldexp(std::fabs(v), -23), std::ldexp(1.0, -25)) * inv;
          range = range && std::fabs(v) < 32768.0;
        }
    expect(back, "x3 (%d, %d, %d): the two planes times 1 / S_w give w", cin, cout, k);
    expect(range, "x3 (%d, %d, %d): |w * S_w| < 2^15", cin, cout, k);
    expect(first == N && only_named(buf, named), "x3 (%d, %d, %d): every element once", cin, cout, k);
  }
}

// the two whole-ResBlock streams, rearranged from per-conv channels-last streams as the packer does
static void check_streams(int C, int k, int nd, bool pair) {
  const int64_t units = pair ? rb16_stream_units(k, nd) : rbcl_stream_units(C, k, nd);
  const int brow = pair ? kRb16BiasRow : kRbclBiasRow;
  std::vector<uint16_t> stream((size_t)units * 512, 0);
  std::vector<float> bias((size_t)2 * nd * brow, 0.f);
  std::vector<std::vector<float>> ws;
  for (int s = 0; s < 2 * nd; ++s) {
    ws.push_back(dense(C, C, k, s));
    const std::vector<float>& w = ws.back();
    std::vector<uint16_t> cl((size_t)cl_w_elems(C, round_up(C, 32), k), 0);
    pack_cl_bf16(cl.data(), C, C, k, [&](int co, int ci, int j) { return w[((size_t)co * C + ci) * k + j]; });
    if (pair) rb16_put_conv(stream.data(), bias.data(), s, cl.data(), w.data(), k);
    else rbcl_put_conv(stream.data(), bias.data(), s, cl.data(), w.data(), C, k);
  }
  bool back = true, bok = true;
  const int G = C / 16;
  for (int s = 0; s < 2 * nd; ++s) {
    for (int co = 0; co < C; ++co) {
      bok = bok && bias[(size_t)s * brow + co] == ws[s][(size_t)co];
      for (int ci = 0; ci < C; ++ci)
        for (int j = 0; j < k; ++j) {
          const int64_t at = pair ? (int64_t)s * rb16_units(k) * 512 + rb16_w_index(j, ci, co)
                                  : ((int64_t)s * resblock_cl_bf16_units(C, k) + (int64_t)j * G + ci / 16) * 512 + cl_w_index(j, ci, co, C, k) % 512;
          back = back && stream[(size_t)at] == f2bf(ws[s][((size_t)co * C + ci) * k + j]);
        }
    }
  }
  expect(back, pair ? "tap-pair stream C = %d, k = %d, nd = %d: read back" : "tap-major stream C = %d, k = %d, nd = %d: read back", C, k, nd);
  expect(nonzero(stream) == (int64_t)2 * nd * C * C * k, "whole-ResBlock stream C = %d, k = %d, nd = %d: every element once", C, k, nd);
  expect(bok && nonzero(bias) == (int64_t)2 * nd * C, "whole-ResBlock bias C = %d, k = %d, nd = %d", C, k, nd);
}

int main() {
  const int f32[4][3] = {{16, 1, 1}, {20, 29, 1}, {16, 33, 3}, {192, 96, 5}};      // (cin, cout, k): every padding rule bites
  for (auto& s : f32) check_f32(s[0], s[1], s[2]);
  const int cl[4][3] = {{16, 16, 3}, {32, 32, 7}, {32, 64, 11}, {64, 16, 1}};
  for (auto& s : cl) check_cl(s[0], s[1], s[2]);
  for (int C : {16, 32})
    for (int k : {3, 11}) check_streams(C, k, 3, false);
  for (int k : {3, 7, 11}) check_streams(16, k, 3, true);
  std::printf(fails ? "%d check(s) failed\n" : "pack_formats_check: all checks passed\n", fails);
  return fails ? 1 : 0;
}
