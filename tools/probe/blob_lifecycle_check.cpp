// blob_lifecycle_check.cpp — the host half of the three packed weight blobs' lifecycle (bv2_api.cpp, bv2_model.cpp) driven through the C API
// by a program of its own, so that it can run under host sanitizers without anything being loaded into Python and without a GPU:
//
//   K=bert-vits2_amd/csrc
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -x hip -Xarch_host -fsanitize=address,undefined -Iinclude \
//         tools/probe/blob_lifecycle_check.cpp $K/bv2_api.cpp $K/bv2_model.cpp $K/kernels/resblock_cl_bf16.hip \
//         $K/kernels/resblock_c16_bf16.hip $K/kernels/dds_fused.hip -Wl,--unresolved-symbols=ignore-all -o /tmp/blob_lifecycle_check
//   /tmp/blob_lifecycle_check
//
// (The three kernel files define the host-side predicates the layout asks; the executors and launchers bv2_api.cpp names stay unresolved and
// are never reached: nothing here attaches a blob or runs a call.  That is the hazard of this way of linking: the linker reports nothing, so
// a change that makes create / load / size / pack reach another translation unit shows here as a jump to address 0 when the program runs,
// not as a link error — then add that file to the build line, or give its function a stub in this program.)
// For each kind on a tiny WN-flow config: create, size, pack with nothing loaded (refused, names the tensors), then let the refusals dictate
// the tensors — a named key is loaded as a scalar, the shape mismatch that follows says the shape, the tensor is loaded again in turn as
// F32, F16 and BF16 — until the pack succeeds; the short buffer is refused, a second pack gives the same bytes, the header is the kind's.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../bert-vits2_amd/csrc/bv2_pack.h"

using namespace bv2;

static int fails = 0;
static void expect(bool ok, const char* kind, const char* what) {
  if (ok) return;
  std::printf("FAIL: %s: %s\n", kind, what);
  ++fails;
}

struct KindFns {
  const char* name;
  uint32_t magic, layout;
  int (*load)(bv2_handle*, const char*, const void*, const int64_t*, int, int);
  int64_t (*size)(bv2_handle*);
  int (*pack)(bv2_handle*, void*, int64_t);
  const char *own, *foreign;
};
static const int kSpec = 80;
static const KindFns kKinds[3] = {
    {"inference", kBlobMagic, BV2_PACK_LAYOUT, bv2_load_tensor, [](bv2_handle* h) { return bv2_packed_bytes(h); }, bv2_pack_weights,
     "enc_p.emb.weight", "enc_q.pre.bias"},
    {"posterior", kPosteriorMagic, BV2_POSTERIOR_LAYOUT, bv2_posterior_load_tensor, [](bv2_handle* h) { return bv2_posterior_packed_bytes(h, kSpec); },
     [](bv2_handle* h, void* b, int64_t n) { return bv2_posterior_pack(h, kSpec, b, n); }, "enc_q.pre.bias", "sdp.post_pre.bias"},
    {"sdp_forward", kSdpForwardMagic, BV2_SDP_FORWARD_LAYOUT, bv2_sdp_forward_load_tensor, bv2_sdp_forward_packed_bytes, bv2_sdp_forward_pack,
     "sdp.post_pre.bias", "dec.conv_pre.bias"},
};

// one tensor of `shape` under `key`, values a function of the element index, handed over as `dtype`
static int load(const KindFns& k, bv2_handle* h, const std::string& key, const std::vector<int64_t>& shape, int dtype) {
  int64_t n = 1;
  for (int64_t d : shape) n *= d;
  std::vector<float> f((size_t)n);
  for (int64_t i = 0; i < n; ++i) f[(size_t)i] = 0.25f + (float)((i * 37 + (int64_t)key.size()) % 101) * 0.0078125f;
  std::vector<uint16_t> s((size_t)n);
  for (int64_t i = 0; i < n; ++i) s[(size_t)i] = dtype == BV2_F16 ? f2h(f[(size_t)i]) : f2bf(f[(size_t)i]);
  const void* p = dtype == BV2_F32 ? static_cast<const void*>(f.data()) : static_cast<const void*>(s.data());
  return k.load(h, key.c_str(), p, shape.data(), (int)shape.size(), dtype);
}

static void run(const KindFns& k, const bv2_config& cfg) {
  bv2_handle* h = nullptr;
  if (bv2_create(&cfg, &h)) { std::printf("FAIL: bv2_create: %s\n", bv2_last_error(nullptr)); ++fails; return; }
  const int64_t n = k.size(h);
  expect(n > 0 && n % 4 == 0, k.name, "size");
  std::vector<unsigned char> blob((size_t)n), again((size_t)n);                // exactly the stated size: a write past it is the sanitizer's to find
  const float one = 1.f;
  const int64_t one_shape = 1;
  expect(k.load(h, k.foreign, &one, &one_shape, 1, BV2_F32) == 1, k.name, "a foreign key is answered with 1");
  expect(k.load(h, nullptr, &one, &one_shape, 1, BV2_F32) == -1 && k.load(h, k.own, nullptr, &one_shape, 1, BV2_F32) == -1 &&
             k.load(h, k.own, &one, &one_shape, 9, BV2_F32) == -1 && k.load(h, k.own, &one, &one_shape, 1, 7) == -1,
         k.name, "bad arguments are refused");
  int rc = k.pack(h, blob.data(), n);
  expect(rc == -2 && std::strstr(bv2_last_error(h), "missing/invalid tensors"), k.name, "a pack with nothing loaded names the missing tensors");
  int loaded = 0, packs = 1;
  while (rc == -2 && packs < 4000) {
    // "...: key; key (shape mismatch: got [..] want [a,b,]); "
    std::string e = bv2_last_error(h);
    size_t at = e.find("): ");
    if (at == std::string::npos) break;
    at += 3;
    while (at < e.size()) {
      const size_t end = e.find("; ", at);
      if (end == std::string::npos) break;
      const std::string item = e.substr(at, end - at);
      at = end + 2;
      const size_t sp = item.find(" (shape mismatch");
      std::vector<int64_t> shape;                                              // a key named for the first time goes in as a scalar
      if (sp != std::string::npos) {
        const size_t w = item.find("want [", sp) + 6;
        for (const char* p = item.c_str() + w; *p && *p != ']';) {
          char* q;
          shape.push_back(std::strtoll(p, &q, 10));
          p = *q == ',' ? q + 1 : q;
        }
      }
      expect(load(k, h, item.substr(0, sp), shape, loaded % 3) == 0, k.name, "an own tensor is taken");
      loaded += sp != std::string::npos;
    }
    rc = k.pack(h, blob.data(), n);
    ++packs;
  }
  expect(rc == 0, k.name, rc == -2 ? bv2_last_error(h) : "the pack succeeds once every tensor is there");
  expect(k.pack(h, again.data(), n - 1) == -1 && std::strstr(bv2_last_error(h), "too small"), k.name, "a buffer one byte short is refused");
  expect(k.pack(h, again.data(), n) == 0 && blob == again, k.name, "packing is a pure function of the tensors");
  uint32_t hdr[8];
  std::memcpy(hdr, blob.data(), sizeof(hdr));
  int64_t tf;
  std::memcpy(&tf, hdr + 4, sizeof(tf));
  expect(hdr[0] == k.magic && hdr[1] == BV2_ABI_VERSION && hdr[3] == k.layout && tf * 4 == n, k.name, "header");
  std::printf("%-11s %9lld bytes, %d tensors in %d packs\n", k.name, (long long)n, loaded, packs);
  bv2_destroy(h);
}

int main() {
  bv2_config c;
  std::memset(&c, 0, sizeof(c));
  c.struct_bytes = (int32_t)sizeof(c);
  c.n_vocab = 4; c.n_tones = 2; c.n_languages = 2; c.bert_dim = 8;
  c.inter_channels = 64; c.hidden_channels = 128; c.filter_channels = 128;
  c.n_heads = 4; c.n_layers = 3; c.kernel_size = 3;
  c.gin_channels = 64; c.n_speakers = 2;
  c.use_transformer_flow = 0; c.n_flow_layer = 2; c.n_layers_trans_flow = 3;
  c.n_upsamples = 2; c.upsample_initial_channel = 64;
  for (int i = 0; i < 2; ++i) { c.upsample_rates[i] = 2; c.upsample_kernel_sizes[i] = 4; }
  c.n_resblock_kernels = 1; c.n_resblock_dilations = 3; c.resblock_type = 1;
  c.resblock_kernel_sizes[0] = 3;
  for (int d = 0; d < 3; ++d) c.resblock_dilation_sizes[0][d] = 1 + 2 * d;
  for (const KindFns& k : kKinds) run(k, c);
  std::printf(fails ? "%d check(s) failed\n" : "blob_lifecycle_check: all checks passed\n", fails);
  return fails ? 1 : 0;
}
