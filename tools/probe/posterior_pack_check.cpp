// posterior_pack_check.cpp — the host side of the posterior encoder's packer (bv2_model.cpp: build_posterior_layout, pack_posterior_blob)
// driven by a program of its own, so that it can run under host sanitizers without anything being loaded into Python and without a GPU:
//
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -x hip -Xarch_host -fsanitize=address,undefined -Iinclude \
//         tools/probe/posterior_pack_check.cpp bert-vits2_amd/csrc/bv2_model.cpp -Wl,--unresolved-symbols=ignore-all -o /tmp/posterior_pack_check
//   /tmp/posterior_pack_check
//
// (bv2_model.cpp's inference packer refers to helpers of other translation units; this program never reaches them, hence the linker flag —
// with it a newly reached helper is a jump to address 0 at run time, not a link error.)
// It packs seeded tensors for the three accepted spectrogram widths in both weight-norm forms, checks the header, that every weight landed
// exactly once (sum of squares), that a missing and a misshapen tensor are reported, and that a bad width is refused.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <random>
#include <string>
#include <vector>

#include "../../bert-vits2_amd/csrc/bv2_internal.h"

using namespace bv2;

static HostTensor tensor(std::mt19937& rng, std::vector<int64_t> shape, float std) {
  HostTensor t;
  t.shape = shape;
  int64_t n = 1;
  for (auto d : shape) n *= d;
  t.data.resize((size_t)n);
  std::normal_distribution<float> N(0.f, std);
  for (auto& v : t.data) v = N(rng);
  return t;
}

int main() {
  bv2_config c;
  std::memset(&c, 0, sizeof(c));
  c.struct_bytes = sizeof(c);
  c.hidden_channels = 192; c.inter_channels = 192; c.gin_channels = 256; c.n_speakers = 10;
  int fails = 0;
  auto expect = [&](bool ok, const char* what) { if (!ok) { std::printf("FAIL: %s\n", what); ++fails; } };
  const int H = c.hidden_channels, C = c.inter_channels, G = c.gin_channels, nl = kPosteriorLayers;
  for (int spec : {1025, 513, 80}) {
    for (int folded = 0; folded < 2; ++folded) {
      std::mt19937 rng(7u + (unsigned)spec);
      WeightBlob b;                                               // the handle's record of this blob: tensors in, length and hash out
      std::map<std::string, HostTensor>& T = b.tensors;
      double want = 0;                                            // sum of squares of every packed weight and bias
      auto plain = [&](const std::string& k, std::vector<int64_t> s, float sd) {
        T[k] = tensor(rng, s, sd);
        for (float v : T[k].data) want += (double)v * v;
      };
      auto normed = [&](const std::string& p, int d0, int d1, int k) {
        HostTensor v = tensor(rng, {d0, d1, k}, 1.f), g = tensor(rng, {d0, 1, 1}, 0.1f);
        HostTensor w = v;
        const int64_t inner = (int64_t)d1 * k;
        for (int a = 0; a < d0; ++a) {
          g.data[a] = 0.7f + g.data[a];
          double ss = 0;
          for (int64_t i = 0; i < inner; ++i) ss += (double)v.data[a * inner + i] * v.data[a * inner + i];
          const float sc = g.data[a] / (float)std::sqrt(ss);
          for (int64_t i = 0; i < inner; ++i) { w.data[a * inner + i] = v.data[a * inner + i] * sc; want += (double)w.data[a * inner + i] * w.data[a * inner + i]; }
        }
        if (folded) T[p + ".weight"] = w;
        else { T[p + ".weight_v"] = v; T[p + ".weight_g"] = g; }
        plain(p + ".bias", {d0}, 0.02f);
      };
      plain("enc_q.pre.weight", {H, spec, 1}, 0.03f); plain("enc_q.pre.bias", {H}, 0.02f);
      normed("enc_q.enc.cond_layer", 2 * H * nl, G, 1);
      for (int i = 0; i < nl; ++i) {
        normed("enc_q.enc.in_layers." + std::to_string(i), 2 * H, H, 5);
        normed("enc_q.enc.res_skip_layers." + std::to_string(i), i < nl - 1 ? 2 * H : H, H, 1);
      }
      plain("enc_q.proj.weight", {2 * C, H, 1}, 0.07f); plain("enc_q.proj.bias", {2 * C}, 0.02f);

      PosteriorW W;
      std::string err;
      expect(build_posterior_layout(c, spec, W, b, err) == 0 && b.total_floats > 0, "layout");
      std::vector<float> blob((size_t)b.total_floats, -1.f);      // exactly the advertised size: a write past it is the sanitizer's to find
      expect(pack_posterior_blob(c, W, b, blob.data(), err) == 0, err.c_str());
      uint32_t hdr[4];
      std::memcpy(hdr, blob.data(), sizeof(hdr));
      expect(hdr[0] == kPosteriorMagic && hdr[1] == BV2_ABI_VERSION && hdr[2] == b.cfg_hash && hdr[3] == BV2_POSTERIOR_LAYOUT, "header");
      double got = 0;
      for (size_t i = kBlobHeaderFloats; i < blob.size(); ++i) got += (double)blob[i] * blob[i];
      expect(std::fabs(got - want) <= 1e-6 * want, "every weight exactly once, padding zero");
      std::printf("spec %4d %s: %lld floats, sum of squares %.6f / %.6f\n", spec, folded ? "folded  " : "weight_g/v", (long long)b.total_floats, got, want);

      WeightBlob b2 = b;
      b2.tensors.erase("enc_q.proj.bias");
      expect(pack_posterior_blob(c, W, b2, blob.data(), err) == -2 && err.find("enc_q.proj.bias") != std::string::npos, "missing tensor named");
      b2 = b;
      b2.tensors["enc_q.pre.bias"].shape = {H + 1};
      expect(pack_posterior_blob(c, W, b2, blob.data(), err) == -2 && err.find("shape mismatch") != std::string::npos, "misshapen tensor named");
    }
  }
  PosteriorW W;
  WeightBlob b;
  std::string err;
  expect(build_posterior_layout(c, 1024, W, b, err) != 0 && b.total_floats == 0 && err.find("1025, 513 or 80") != std::string::npos, "bad width refused");
  std::printf(fails ? "%d check(s) failed\n" : "posterior_pack_check: all checks passed\n", fails);
  return fails ? 1 : 0;
}
