"""GPU: the Encoder layer's fused launch forms, each kernel on its own against the fp64 references of tests/encoder_refs.py
(proved against the oracle in tests/test_encoder_forms_cpu.py): the fused conv_o, the key split with its merge in LayerNorm-1, the
fp16 K / V hand-over (both ends), the LayerNorm in the fp16 conv epilogue and the WN gate epilogue.

Every buffer a kernel writes is NaN (fp16: 0x7e00) before the launch, and so is every padding row or column it must not read.
Tolerances are bounds the suite already holds (test_attention_relpos: 2e-5 fp32 / 4e-3 fp16 of the output scale;
test_layernorm_family: 1e-5; test_conv_f16_kernel: 3e-5, 2^-10 per fp16 store), propagated through a LayerNorm where its input
carries a kernel's error: d out = rstd * gamma * d in at most.  Each test prints its measured figure before it asserts."""
import ctypes as C
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from tests import encoder_refs as R

pytestmark = pytest.mark.gpu

W = R.WINDOW
NR = 2 * W + 1
_vp, _i, _i64 = C.c_void_p, C.c_int, C.c_int64

_ATTN = [("stream", _vp), ("qkv", _vp), ("ld", _i), ("mask", _vp), ("erv", _vp), ("out", _vp), ("B", _i), ("H", _i), ("D", _i),
         ("T", _i), ("W", _i), ("f16", _i), ("kh", _vp), ("vh", _vp), ("wo_host", _vp), ("wo_pack_dev", _vp), ("bo", _vp),
         ("res", _vp), ("o_out", _vp), ("o_slab_stride", _i64), ("Co", _i), ("ksplit", _i), ("ml_out", _vp)]
_LN = [("stream", _vp), ("a", _vp), ("add", _vp), ("mode", _i), ("dww", _vp), ("dwb", _vp), ("dil", _i), ("in_mask", _vp),
       ("gamma", _vp), ("beta", _vp), ("post_gelu", _i), ("res", _vp), ("vec", _vp), ("mask", _vp), ("out", _vp), ("B", _i),
       ("C", _i), ("T", _i), ("nslab", _i), ("slab_stride", _i64), ("ml", _vp), ("ml_H", _i), ("ml_ks", _i), ("bias", _vp),
       ("out2", _vp), ("vec2", _vp), ("pf_ptr", _vp), ("pf_bytes", C.c_uint)]
_HC = [("stream", _vp), ("x", _vp), ("in_ct", _i), ("in_mask", _vp), ("w_host", _vp), ("bias_host", _vp), ("wpack_dev", _vp),
       ("out", _vp), ("out_ct", _i), ("res", _vp), ("res_mode", _i), ("out_mask", _vp), ("mask_pre", _i), ("mask_post", _i),
       ("act", _i), ("B", _i), ("cin", _i), ("cout", _i), ("k", _i), ("dil", _i), ("L", _i), ("out_rstride", _i),
       ("ln_gamma", _vp), ("ln_beta", _vp), ("ln_vec", _vp), ("ln_mask", _vp), ("k16", _vp), ("v16", _vp), ("kv_row0", _i),
       ("kv_rows", _i), ("k16_ld", _i), ("bias2", _vp), ("bias2_bstride", _i), ("no_ksplit", _i), ("p1_w_host", _vp),
       ("p1_bias_host", _vp), ("p1_out", _vp), ("p1_res", _vp), ("p1_res_mode", _i)]


@functools.lru_cache(maxsize=None)
def _lib():
    from bert_vits2_amd import lib as L
    lib = L.load()
    for name, spec in (("bv2_test_attention_ex", _ATTN), ("bv2_test_layernorm_ex", _LN), ("bv2_test_conv_f16_ex", _HC)):
        fn = getattr(lib, name)
        fn.restype = C.c_int
        fn.argtypes = [t for _, t in spec]
    lib.bv2_test_conv_cl_pack_bytes.restype = C.c_int64
    lib.bv2_test_conv_cl_pack_bytes.argtypes = [C.c_int] * 3
    lib.bv2_test_set_variants.restype = None
    lib.bv2_test_set_variants.argtypes = [C.c_char_p, C.c_int, C.c_int]
    return lib


def _call(name, spec, **kw):
    """One launcher call by argument name: tensors become their data pointers, what is not named is NULL / 0."""
    unknown = set(kw) - {n for n, _ in spec}
    assert not unknown, unknown
    args = []
    for n, t in spec:
        v = kw.get(n)
        if t is _vp:
            args.append(None if v is None else C.c_void_p(v.data_ptr()))
        else:
            args.append(0 if v is None else v)
    rc = getattr(_lib(), name)(*args)
    torch.cuda.synchronize()
    return rc


def attention_ex(**kw):
    return _call("bv2_test_attention_ex", _ATTN, **kw)


def layernorm_ex(**kw):
    return _call("bv2_test_layernorm_ex", _LN, **kw)


def conv_f16_ex(**kw):
    return _call("bv2_test_conv_f16_ex", _HC, **kw)


def nanf(*shape):
    return torch.full(shape, float("nan"), device="cuda")


def nanh(*shape):
    return torch.full(shape, 0x7E00, dtype=torch.int16, device="cuda").view(torch.float16)


def is_nanh(t):
    return t.contiguous().view(torch.int16) == 0x7E00


def h16(t):
    return t.to(torch.float16).to(torch.float32)


def r32(n):
    return (n + 31) // 32 * 32


def len_mask(lens, T):
    return (torch.arange(T)[None, :] < torch.tensor(lens)[:, None]).float()


def pack_qkv(qs, kv, erk, H, D, T, kv_nan=False):
    """The attention kernel's input rows [q / sqrt(D) | k | v | per head the 2W+1 relative-key logits], row stride ld (32-aligned), the
    padding columns NaN; kv_nan: the k and v rows entirely NaN (the fp16 hand-over must not read them)."""
    B = qs.shape[0]
    ld = r32(T)
    qe = torch.einsum("bhdt,rd->bhrt", qs.view(B, H, D, T), erk).reshape(B, H * NR, T)
    packed = torch.full((B, 3 * H * D + H * NR, ld), float("nan"))
    packed[:, :, :T] = torch.cat([qs, kv, qe], 1)
    if kv_nan:
        packed[:, H * D: 3 * H * D] = float("nan")
    return packed.cuda(), ld


@functools.lru_cache(maxsize=None)
def _case(B, T, lens, H, D, qmul):
    """Inputs and the unsplit fp64 attention of a case: computed once per module, read-only."""
    qkv, erk, erv, mask = R.attention_inputs(B, T, lens, H, D, qmul)
    return dict(qkv=qkv, erk=erk, erv=erv, mask=mask, att=R.ref_attention(qkv, mask, erk, erv, H, W))


def _launch_fused(c, B, T, H, D, Co, wo, bo=None, res=None, ks=1):
    HD = H * D
    packed, ld = pack_qkv(c["qkv"][:, :HD] / math.sqrt(D), c["qkv"][:, HD:], c["erk"], H, D, T)
    slabs, out = nanf(H * ks, B, Co, T), nanf(B, HD, T)
    ml = nanf(B, H, ks, 2, T) if ks > 1 else None
    wp = torch.empty(r32(Co) * ((HD + 15) // 16 * 16), device="cuda")
    dev = lambda t: None if t is None else t.cuda()
    bo_d, res_d, mk, ev = dev(bo), dev(res), c["mask"].cuda(), c["erv"].cuda()
    rc = attention_ex(qkv=packed, ld=ld, mask=mk, erv=ev, out=out, B=B, H=H, D=D, T=T, W=W, wo_host=wo, wo_pack_dev=wp, bo=bo_d,
                      res=res_d, o_out=slabs, o_slab_stride=B * Co * T, Co=Co, ksplit=ks, ml_out=ml)
    assert torch.isnan(out).all()                          # the plain output is not written by the fused form
    return rc, slabs.cpu().double(), None if ml is None else ml.cpu().double()


# ------------------------------------------------------------------------------------------------------------------
# a. fused conv_o (fp32, no split)

@pytest.mark.parametrize("H,D,Co", [(2, 96, 192), (4, 32, 96), (1, 128, 160)])   # Co <= 128: the 4-wave variant at T <= 128; 160: a half-empty last row tile
@pytest.mark.parametrize("B,T,lens", [(1, 128, (128,)), (2, 100, (100, 37)), (1, 33, (33,)), (1, 300, (300,)), (1, 3, (3,))])
def test_fused_conv_o(B, T, lens, H, D, Co):
    """The sum of the H head slabs is conv_o(attention) + bias + residual; bias and residual ride on slab 0 alone."""
    c = _case(B, T, lens, H, D, 3.0)
    wo, bo, res = R.conv_o_weights(H, D, Co, B, T)
    ref = R.ref_conv_o(c["att"], wo, bo, res)
    rc, slabs, _ = _launch_fused(c, B, T, H, D, Co, wo, bo, res)
    assert rc == 0
    assert torch.isfinite(slabs).all()
    valid = c["mask"][:, None, :].bool().expand_as(ref)
    err, bound = (slabs.sum(0) - ref).abs()[valid].max().item(), 2e-5 * ref.abs().max().item()
    print(f"\n[a H={H} D={D} Co={Co} T={T}] slab sum: max err {err:.3e} (bound {bound:.3e})")
    assert err <= bound
    if H > 1:
        head1 = R.ref_conv_o(c["att"][:, D:2 * D], wo[:, D:2 * D])
        err1, bound1 = (slabs[1] - head1).abs()[valid].max().item(), 2e-5 * head1.abs().max().item()
        print(f"[a] slab 1 against head 1's projection: max err {err1:.3e} (bound {bound1:.3e})")
        assert err1 <= bound1


# ------------------------------------------------------------------------------------------------------------------
# b. key split

_B_WORST = {}


def _split_launch(B, T, lens, H, D, ks, qmul, Co=192):
    c = _case(B, T, lens, H, D, qmul)
    wo, bo, res = R.conv_o_weights(H, D, Co, B, T)
    rc, slabs, ml = _launch_fused(c, B, T, H, D, Co, wo, ks=ks)
    assert rc == 0
    assert torch.isfinite(slabs).all() and torch.isfinite(ml).all()
    return c, wo, bo, res, slabs.view(H, ks, B, Co, T), ml


@pytest.mark.parametrize("B,T,lens,H,D,ks,qmul", R.SPLIT_CASES)
def test_key_split_attention(B, T, lens, H, D, ks, qmul):
    """The kernel alone: its slabs and (max, sum) pairs merged in fp64 by ref_split_merge are the unsplit fp64 result, and the
    pairs themselves are each key range's logit maximum (absolute) and sum of exponentials (relative) for every valid query.

    Bounds of the pairs: a logit is a D-term fp32 dot product, held to 2e-5 of the logit scale s_max (largest unmasked |logit|) like
    every fp32 sum of this suite; an error d of the logits moves each exp(s - m) by a factor e^d, so the sum by d relatively, plus
    1e-5 for the exponentials and their fp32 sum (|s - m| < 88 wherever the term is not 0)."""
    c, wo, bo, res, slabs, ml = _split_launch(B, T, lens, H, D, ks, qmul)
    ref = R.ref_conv_o(c["att"], wo, bo, res)
    got = R.ref_split_merge(slabs, ml[:, :, :, 0], ml[:, :, :, 1]) + bo.double()[None, :, None] + res.double()
    valid = c["mask"][:, None, :].bool().expand_as(ref)
    assert torch.isfinite(got).all()
    err, bound = (got - ref).abs()[valid].max().item(), 2e-5 * ref.abs().max().item()
    print(f"\n[b T={T} lens={lens} H={H} D={D} ks={ks} q x{qmul}] merged in fp64: max err {err:.3e} (bound {bound:.3e})")
    assert err <= bound
    logits = R.ref_logits(c["qkv"], c["mask"], c["erk"], H, W)
    smax = logits[logits > -9999.0].abs().max().item()
    vq = c["mask"][:, None, :].bool().expand(B, H, T)
    for r, (k0, k1) in enumerate(R.key_ranges(T, ks)):
        s = logits[..., k0:k1]
        m_ref = s.max(-1).values
        l_ref = torch.exp(s - m_ref[..., None]).sum(-1)
        m, l = ml[:, :, r, 0], ml[:, :, r, 1]
        em = (m - m_ref).abs()[vq].max().item()
        el = ((l * torch.exp(m - m_ref) - l_ref).abs() / l_ref)[vq].max().item()
        print(f"[b] range {r} keys [{k0}, {k1}): max |m - ref| {em:.3e} (bound {2e-5 * smax:.3e}), max rel err of l {el:.3e} (bound {2e-5 * smax + 1e-5:.3e})")
        assert em <= 2e-5 * smax
        assert el <= 2e-5 * smax + 1e-5
    if lens == (256, 40):                                   # ranges 2 and 3 of item 1: every key masked for its valid queries
        assert (ml[1, :, 2:, 0, :40] == -1e4).all() and (ml[1, :, 2:, 1, :40] == 64.0).all()


@pytest.mark.parametrize("B,T,lens,H,D,ks,qmul", R.SPLIT_CASES)
def test_key_split_attention_and_layernorm(B, T, lens, H, D, ks, qmul):
    """Kernel + LayerNorm-1 (the flash-decoding merge, conv_o's bias and the residual in the LayerNorm) against fp64
    LN(x + conv_o(attention) + b_o).  The LayerNorm's input carries the attention's error d <= 2e-5 max|pre-LN|, which the
    LayerNorm passes on times rstd * gamma at most; its own bar is 1e-5 of the output scale (test_layernorm_family)."""
    Co = 192
    c, wo, bo, res, slabs, ml = _split_launch(B, T, lens, H, D, ks, qmul, Co)
    g = torch.Generator().manual_seed(T + ks)
    gamma, beta = torch.randn(Co, generator=g), torch.randn(Co, generator=g)
    pre = R.ref_conv_o(c["att"], wo, bo, res)
    ref, rstd = R.ref_layer_norm(pre, gamma, beta, with_rstd=True)
    out = nanf(B, Co, T)
    t = [x.cuda() for x in (slabs.float(), ml.float(), res, bo, gamma, beta)]
    assert layernorm_ex(a=t[0], add=t[2], gamma=t[4], beta=t[5], out=out, B=B, C=Co, T=T, nslab=H * ks, slab_stride=B * Co * T,
                        ml=t[1], ml_H=H, ml_ks=ks, bias=t[3]) == 0
    got = out.cpu().double()
    assert torch.isfinite(got).all()
    valid = c["mask"][:, None, :].bool().expand_as(ref)
    vcol = c["mask"][:, None, :].bool()
    bound = 1e-5 * ref.abs().max().item() + 2e-5 * pre.abs().max().item() * rstd[vcol].max().item() * gamma.abs().max().item()
    err = (got - ref).abs()[valid].max().item()
    print(f"\n[b+LN T={T} lens={lens} H={H} D={D} ks={ks} q x{qmul}] max err {err:.3e} (bound {bound:.3e})")
    assert err <= bound


def test_attention_launcher_contract():
    """Refused combinations return -1 and launch nothing."""
    B, T, H, D, Co = 1, 65, 2, 96, 192
    c = _case(B, T, (65,), H, D, 3.0)
    wo, bo, res = R.conv_o_weights(H, D, Co, B, T)
    for kw in (dict(ks=4), dict(ks=2, bo=bo), dict(ks=2, res=res)):          # more ranges than the 3 key tiles; bias / residual with a split
        rc, slabs, ml = _launch_fused(c, B, T, H, D, Co, wo, **kw)
        assert rc == -1
        assert torch.isnan(slabs).all() and torch.isnan(ml).all()
    packed, ld = pack_qkv(c["qkv"][:, : H * D] / math.sqrt(D), c["qkv"][:, H * D:], c["erk"], H, D, T)
    out, kh, vh = nanf(B, H * D, T), nanh(B, ld, H * D), nanh(B, H * D, ld)
    mk, ev = c["mask"].cuda(), c["erv"].cuda()
    base = dict(qkv=packed, ld=ld, mask=mk, erv=ev, out=out, B=B, H=H, D=D, T=T, W=W)
    assert attention_ex(f16=0, kh=kh, vh=vh, **base) == -1                     # fp16 K / V without the fp16 products
    assert attention_ex(f16=1, kh=kh, **base) == -1                            # K without V
    assert attention_ex(f16=1, vh=vh, **base) == -1
    assert torch.isnan(out).all()


# ------------------------------------------------------------------------------------------------------------------
# c. the weighted-slab LayerNorm on its own

def _weighted_case(C_, T, H, ks, spread, B=2, seed=0):
    g = torch.Generator().manual_seed(C_ + T + 10 * H + ks + int(spread) + seed)
    ns = H * ks
    slabs = torch.randn(ns, B, C_, T, generator=g)
    m = torch.randn(B, H, 1, T, generator=g) * 3 + spread * torch.rand(B, H, ks, T, generator=g)
    l = 1 + 63 * torch.rand(B, H, ks, T, generator=g)
    m[0, H - 1], l[0, H - 1] = -1e4, 32.0                  # a fully masked row: every range (-1e4, 32)
    ml = torch.stack([m, l], 3).contiguous()               # [B][H][ks][2][T]
    add, bias = torch.randn(B, C_, T, generator=g), torch.randn(C_, generator=g)
    gamma, beta = torch.randn(C_, generator=g), torch.randn(C_, generator=g)
    vec, vec2 = torch.randn(B, C_, generator=g), torch.randn(B, C_, generator=g)
    mask = len_mask([T, max(1, T - 3)][:B], T)
    pre = R.ref_split_merge(slabs.view(H, ks, B, C_, T), m, l) + bias.double()[None, :, None] + add.double()
    return dict(slabs=slabs, ml=ml, add=add, bias=bias, gamma=gamma, beta=beta, vec=vec, vec2=vec2, mask=mask, pre=pre)


def _weighted_launch(w, B, C_, T, H, ks, out, **extra):
    t = {k: w[k].cuda() for k in ("slabs", "ml", "add", "bias", "gamma", "beta", "vec", "mask")}
    rc = layernorm_ex(a=t["slabs"], add=t["add"], gamma=t["gamma"], beta=t["beta"], vec=t["vec"], mask=t["mask"], out=out, B=B, C=C_, T=T,
                      nslab=H * ks, slab_stride=B * C_ * T, ml=t["ml"], ml_H=H, ml_ks=ks, bias=t["bias"], **extra)
    assert rc == 0


@pytest.mark.parametrize("spread", [0.0, 5.0, 200.0])
@pytest.mark.parametrize("H,ks", [(2, 2), (1, 4), (4, 2), (2, 4)])               # nslab / ks = 4/2, 4/4, 8/2, 8/4: the four instantiations
@pytest.mark.parametrize("C_,T", [(192, 5), (192, 77), (256, 5), (256, 77)])
def test_weighted_slab_layernorm(C_, T, H, ks, spread):
    """LayerNorm of sum_{h,r} w_{h,r} slab + bias + add with random (max, sum) pairs — maxima 0, 5 and 200 apart (200: weights that
    underflow to 0 in fp32) and one fully masked head — against ref_split_merge + LayerNorm in fp64, input given exactly."""
    B = 2
    w = _weighted_case(C_, T, H, ks, spread)
    ref = R.ref_ln_vec_mask(w["pre"], w["gamma"], w["beta"], w["vec"], w["mask"])
    out = nanf(B, C_, T)
    _weighted_launch(w, B, C_, T, H, ks, out)
    got = out.cpu().double()
    assert torch.isfinite(got).all()
    err = ((got - ref).abs().max() / ref.abs().max()).item()
    print(f"\n[c C={C_} T={T} nslab={H * ks} ks={ks} spread={spread}] rel err {err:.3e} (bound 1e-5)")
    assert err <= 1e-5


def test_weighted_slab_layernorm_second_output():
    """out2 = (LN + vec + vec2) * mask next to out = (LN + vec) * mask."""
    B, C_, T, H, ks = 2, 192, 77, 2, 4
    w = _weighted_case(C_, T, H, ks, 5.0, seed=1)
    ref = R.ref_ln_vec_mask(w["pre"], w["gamma"], w["beta"], w["vec"], w["mask"])
    ref2 = R.ref_ln_vec_mask(w["pre"], w["gamma"], w["beta"], w["vec"] + w["vec2"], w["mask"])
    out, out2, v2 = nanf(B, C_, T), nanf(B, C_, T), w["vec2"].cuda()
    _weighted_launch(w, B, C_, T, H, ks, out, out2=out2, vec2=v2)
    for got, want in ((out, ref), (out2, ref2)):
        got = got.cpu().double()
        assert torch.isfinite(got).all()
        err = ((got - want).abs().max() / want.abs().max()).item()
        print(f"\n[c out/out2] rel err {err:.3e} (bound 1e-5)")
        assert err <= 1e-5


def test_weighted_slab_layernorm_prefetch_grid():
    """B = 1 with a weight prefetch of 1000 bytes (not a multiple of the 128-byte line): the tiles are padded to a multiple of 8 and
    spare workgroups touch the buffer.  Same bits as the launch without it; the buffer and what follows it are only read."""
    B, C_, T, H, ks = 1, 192, 77, 2, 4
    w = _weighted_case(C_, T, H, ks, 5.0, B=1, seed=2)
    ref = R.ref_ln_vec_mask(w["pre"], w["gamma"], w["beta"], w["vec"], w["mask"])
    plain, withpf = nanf(B, C_, T), nanf(B, C_, T)
    pf = nanf(1024)                                         # 1000 bytes of "weights" + a guard region, all NaN
    before = pf.view(torch.int32).clone()
    _weighted_launch(w, B, C_, T, H, ks, plain)
    _weighted_launch(w, B, C_, T, H, ks, withpf, pf_ptr=pf, pf_bytes=1000)
    assert torch.equal(pf.view(torch.int32), before)
    assert torch.isfinite(withpf).all()
    assert torch.equal(withpf.view(torch.int32), plain.view(torch.int32))
    assert ((plain.cpu().double() - ref).abs().max() / ref.abs().max()).item() <= 1e-5


# ------------------------------------------------------------------------------------------------------------------
# d. attention on fp16 K / V handed over by the projection

@functools.lru_cache(maxsize=None)
def _kv16_case(B, T, lens, H, D):
    HD = H * D
    qkv, erk, erv, mask = R.attention_inputs(B, T, lens, H, D, 3.0)
    qs = h16(qkv[:, :HD] / math.sqrt(D))                   # what the kernel rounds q / sqrt(D) to: already an fp16 number
    k, v = h16(qkv[:, HD:2 * HD]), h16(qkv[:, 2 * HD:])
    ref = R.ref_attention(torch.cat([qs.double() * math.sqrt(D), k.double(), v.double()], 1), mask, erk, erv, H, W)
    return dict(qs=qs, k=k, v=v, erk=erk, erv=erv, mask=mask, ref=ref)


@pytest.mark.parametrize("H,D", [(2, 96), (8, 32), (3, 64), (2, 128)])
@pytest.mark.parametrize("B,T,lens", [(1, 33, (33,)), (2, 100, (100, 37)), (1, 300, (300,)), (1, 64, (64,))])
def test_attention_kv16(B, T, lens, H, D):
    """K [B][ld][HD] and V [B][HD][ld] as fp16 with NaN tails, the k / v rows of the fp32 input all NaN: they are not read, and no
    tail row or column reaches a sum."""
    c = _kv16_case(B, T, lens, H, D)
    HD = H * D
    packed, ld = pack_qkv(c["qs"], torch.cat([c["k"], c["v"]], 1), c["erk"], H, D, T, kv_nan=True)
    kh, vh = nanh(B, ld, HD), nanh(B, HD, ld)
    kh[:, :T] = c["k"].transpose(1, 2).to(torch.float16).cuda()
    vh[:, :, :T] = c["v"].to(torch.float16).cuda()
    out, mk, ev = nanf(B, HD, T), c["mask"].cuda(), c["erv"].cuda()
    assert attention_ex(qkv=packed, ld=ld, mask=mk, erv=ev, out=out, B=B, H=H, D=D, T=T, W=W, f16=1, kh=kh, vh=vh) == 0
    got, ref = out.cpu().double(), c["ref"]
    assert torch.isfinite(got).all()
    valid = c["mask"][:, None, :].bool().expand_as(ref)
    err, bound = (got - ref).abs()[valid].max().item(), 4e-3 * ref.abs().max().item()
    print(f"\n[d H={H} D={D} T={T} lens={lens}] max err {err:.3e} (bound {bound:.3e})")
    assert err <= bound


# ------------------------------------------------------------------------------------------------------------------
# e. the projection's K / V routing

@pytest.mark.parametrize("cin,cout,kv", [(192, 594, 192), (256, 840, 256)])     # hidden 192 x 2 heads; hidden 256 x 8 heads
def test_projection_kv_routing(cin, cout, kv):
    """The q/k/v projection with its K / V rows routed to fp16 buffers: bit-equal to the fp16 rounding of the unrouted fp32 rows,
    nothing else changed, nothing written outside (the unrouted launch is held to fp64 by test_conv_f16_kernel)."""
    lib = _lib()
    B, T, ld = 2, 77, 96
    g = torch.Generator().manual_seed(cin + cout)
    x = torch.randn(B, cin, T, generator=g)
    w, bias = torch.randn(cout, cin, 1, generator=g) / math.sqrt(cin), torch.randn(cout, generator=g)
    xd = x.cuda()
    wp = torch.empty(lib.bv2_test_conv_cl_pack_bytes(cin, cout, 1), dtype=torch.uint8, device="cuda")
    plain, routed = nanf(B, cout, ld), nanf(B, cout, ld)
    k16, v16 = nanh(B, ld, kv), nanh(B, kv, ld)
    base = dict(x=xd, in_ct=1, w_host=w, bias_host=bias, wpack_dev=wp, out_ct=1, B=B, cin=cin, cout=cout, k=1, dil=1, L=T, out_rstride=ld)
    assert conv_f16_ex(out=plain, **base) == 0
    assert conv_f16_ex(out=routed, k16=k16, v16=v16, kv_row0=kv, kv_rows=kv, k16_ld=ld, **base) == 0
    bits = lambda t: t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)
    assert torch.isfinite(plain[:, :, :T]).all() and torch.isnan(plain[:, :, T:]).all()
    assert torch.equal(bits(k16[:, :T]), bits(plain[:, kv:2 * kv, :T].transpose(1, 2).to(torch.float16)))
    assert torch.equal(bits(v16[:, :, :T]), bits(plain[:, 2 * kv:3 * kv, :T].to(torch.float16)))
    assert is_nanh(k16[:, T:]).all() and is_nanh(v16[:, :, T:]).all()
    assert torch.isnan(routed[:, kv:3 * kv]).all() and torch.isnan(routed[:, :, T:]).all()
    assert torch.equal(bits(routed[:, :kv, :T]), bits(plain[:, :kv, :T]))                 # q rows
    assert torch.equal(bits(routed[:, 3 * kv:, :T]), bits(plain[:, 3 * kv:, :T]))         # relative-key rows


# ------------------------------------------------------------------------------------------------------------------
# f. LayerNorm in the fp16 conv epilogue

_F_LENS = {(1, 33): [33], (2, 200): [200, 77], (3, 5): [5, 1, 3]}


@pytest.mark.parametrize("vec_mask", [0, 1])
@pytest.mark.parametrize("form", ["conv_o", "ffn2_ksplit", "ffn2_no_ksplit", "ffn2_generic"])
@pytest.mark.parametrize("B,L", [(1, 33), (2, 200), (3, 5)])
def test_conv_f16_layernorm_epilogue(B, L, form, vec_mask):
    """out = (LN(conv + bias [* mask] + res) [+ vec]) [* mask] from the conv's epilogue against the fp64 conv of the fp16-rounded
    operands followed by the fp64 LayerNorm.  The LayerNorm's input carries the conv's error d <= 3e-5 max|pre-LN|
    (test_conv_f16_kernel's bar), passed on times rstd * gamma at most, plus 1e-5 of the output scale for the LayerNorm itself."""
    lib = _lib()
    conv_o = form == "conv_o"
    cin, cout, k = (192, 192, 1) if conv_o else (768, 192, 3)
    g = torch.Generator().manual_seed(B * 1000 + L + k)
    x = torch.randn(B, cin, L, generator=g)
    w, bias = torch.randn(cout, cin, k, generator=g) / math.sqrt(cin * k), torch.randn(cout, generator=g)
    res = torch.randn(B, cout, L, generator=g)
    gamma, beta, vec = torch.randn(cout, generator=g), torch.randn(cout, generator=g), torch.randn(B, cout, generator=g)
    mask = len_mask(_F_LENS[(B, L)], L)
    pl = (k - 1) // 2
    y = F.conv1d(F.pad(h16(x).double(), (pl, k - 1 - pl)), h16(w).double(), bias.double())
    if not conv_o:
        y = y * mask[:, None, :].double()                  # mask_pre
    pre = y + res.double()
    _, rstd = R.ref_layer_norm(pre, gamma, beta, with_rstd=True)
    ref = R.ref_ln_vec_mask(pre, gamma, beta, vec if vec_mask else None, mask if vec_mask else None)
    wp = torch.empty(lib.bv2_test_conv_cl_pack_bytes(cin, cout, k), dtype=torch.uint8, device="cuda")
    md, t = mask.cuda(), [v.cuda() for v in (gamma, beta, vec)]
    ln = dict(ln_gamma=t[0], ln_beta=t[1], ln_vec=t[2] if vec_mask else None, ln_mask=md if vec_mask else None)
    common = dict(w_host=w, bias_host=bias, wpack_dev=wp, out_ct=1, res_mode=1, B=B, cin=cin, cout=cout, k=k, dil=1, L=L)
    if conv_o:                                             # fp32 in; out IS the residual's tensor, its rows padded by 3 NaN columns
        ld = L + 3
        buf = nanf(B, cout, ld)
        buf[:, :, :L] = res.cuda()
        xd = x.cuda()
        rc = conv_f16_ex(x=xd, in_ct=1, out=buf, res=buf, out_rstride=ld, **common, **ln)
        assert torch.isnan(buf[:, :, L:]).all()
        got = buf[:, :, :L].cpu().double()
    else:                                                  # fp16 channels-last in, mask before the residual
        xd = x.transpose(1, 2).contiguous().to(torch.float16).cuda()
        out, rd = nanf(B, cout, L), res.cuda()
        try:
            if form == "ffn2_generic":
                lib.bv2_test_set_variants(b"", 0, 1)
            rc = conv_f16_ex(x=xd, in_ct=0, out=out, res=rd, out_rstride=L, out_mask=md, mask_pre=1,
                             no_ksplit=int(form == "ffn2_no_ksplit"), **common, **ln)
        finally:
            lib.bv2_test_set_variants(b"", 0, 0)
        got = out.cpu().double()
    assert rc == 0
    assert torch.isfinite(got).all()
    bound = 1e-5 * ref.abs().max().item() + 3e-5 * pre.abs().max().item() * rstd.max().item() * gamma.abs().max().item()
    err = (got - ref).abs().max().item()
    print(f"\n[f {form} B={B} L={L} vec+mask={vec_mask}] max err {err:.3e} (bound {bound:.3e})")
    assert err <= bound


def test_conv_f16_layernorm_epilogue_contract():
    """The LayerNorm epilogue exists for cout 192 and one problem per launch: anything else is refused, nothing launched."""
    lib = _lib()
    B, L, cin = 1, 33, 192
    g = torch.Generator().manual_seed(3)
    x = torch.randn(B, cin, L, generator=g).cuda()
    for cout, two in ((256, False), (192, True)):
        w, bias = torch.randn(cout, cin, 1, generator=g) / math.sqrt(cin), torch.randn(cout, generator=g)
        gamma, beta = torch.randn(cout, generator=g).cuda(), torch.randn(cout, generator=g).cuda()
        wp = torch.empty(2 * lib.bv2_test_conv_cl_pack_bytes(cin, cout, 1), dtype=torch.uint8, device="cuda")
        out, out1 = nanf(B, cout, L), nanf(B, cout, L)
        extra = dict(p1_w_host=w, p1_bias_host=bias, p1_out=out1) if two else {}
        assert conv_f16_ex(x=x, in_ct=1, w_host=w, bias_host=bias, wpack_dev=wp, out=out, out_ct=1, B=B, cin=cin, cout=cout, k=1, dil=1,
                           L=L, out_rstride=L, ln_gamma=gamma, ln_beta=beta, **extra) == -1
        assert torch.isnan(out).all() and torch.isnan(out1).all()


# ------------------------------------------------------------------------------------------------------------------
# g. the WN gate epilogue and the two-problem launch

@pytest.mark.parametrize("L", [77, 200])
def test_conv_f16_gate(L):
    """out[b][t][16 mt + j] = fp16(tanh(v[32 mt + j]) * sigmoid(v[32 mt + 16 + j])), v = conv + bias + bias2[b]: 2^-10 of the value for
    the fp16 store plus the conv's 3e-5 of max|v| (the gate's slope in v is at most 1)."""
    lib = _lib()
    B, cin, cout, k = 2, 192, 384, 5
    g = torch.Generator().manual_seed(L)
    x = torch.randn(B, cin, L, generator=g)
    w, bias = torch.randn(cout, cin, k, generator=g) / math.sqrt(cin * k), torch.randn(cout, generator=g)
    bias2 = torch.randn(B, cout, generator=g)
    mask = len_mask([L, L - 19], L)
    pl = (k - 1) // 2
    v = F.conv1d(F.pad(h16(x * mask[:, None, :]).double(), (pl, k - 1 - pl)), h16(w).double(), bias.double()) + bias2.double()[:, :, None]
    v4 = v.view(B, cout // 32, 2, 16, L)
    ref = (torch.tanh(v4[:, :, 0]) * torch.sigmoid(v4[:, :, 1])).reshape(B, cout // 2, L)
    wp = torch.empty(lib.bv2_test_conv_cl_pack_bytes(cin, cout, k), dtype=torch.uint8, device="cuda")
    out, xd, md, b2 = nanh(B, L, cout // 2), x.cuda(), mask.cuda(), bias2.cuda()
    assert conv_f16_ex(x=xd, in_ct=1, in_mask=md, w_host=w, bias_host=bias, wpack_dev=wp, out=out, out_ct=0, act=2, B=B, cin=cin,
                       cout=cout, k=k, dil=1, L=L, bias2=b2, bias2_bstride=cout) == 0
    got = out.float().transpose(1, 2).cpu().double()
    assert torch.isfinite(got).all()
    err = (got - ref).abs()
    tol = 2.0 ** -10 * ref.abs() + 3e-5 * v.abs().max().item()
    print(f"\n[g gate L={L}] max err {err.max().item():.3e}, largest err / tol {(err / tol).max().item():.3f}")
    assert bool((err <= tol).all())


@pytest.mark.parametrize("L", [77, 200])
def test_conv_f16_two_problems(L):
    """The res_skip_layers pair in one launch: problem 0 adds into its residual in place, problem 1 into a second tensor, both
    masked; each against its own fp64 conv at test_conv_f16_kernel's bar for fp32 outputs (3e-5 of the output scale)."""
    lib = _lib()
    B, cin, cout = 2, 192, 192
    g = torch.Generator().manual_seed(L + 1)
    x = h16(torch.randn(B, cin, L, generator=g))
    ws = [torch.randn(cout, cin, 1, generator=g) / math.sqrt(cin) for _ in range(2)]
    bs = [torch.randn(cout, generator=g) for _ in range(2)]
    rs = [torch.randn(B, cout, L, generator=g) for _ in range(2)]
    mask = len_mask([L, L - 19], L)
    refs = [(F.conv1d(x.double(), h16(ws[i]).double(), bs[i].double()) + rs[i].double()) * mask[:, None, :].double() for i in range(2)]
    wp = torch.empty(2 * lib.bv2_test_conv_cl_pack_bytes(cin, cout, 1), dtype=torch.uint8, device="cuda")
    xd, md = x.transpose(1, 2).contiguous().to(torch.float16).cuda(), mask.cuda()
    t0, t1 = rs[0].cuda(), rs[1].cuda()
    assert conv_f16_ex(x=xd, in_ct=0, w_host=ws[0], bias_host=bs[0], wpack_dev=wp, out=t0, out_ct=1, res=t0, res_mode=1, out_mask=md,
                       mask_post=1, B=B, cin=cin, cout=cout, k=1, dil=1, L=L, out_rstride=L, p1_w_host=ws[1], p1_bias_host=bs[1],
                       p1_out=t1, p1_res=t1, p1_res_mode=1) == 0
    for i, got in enumerate((t0, t1)):
        got = got.cpu().double()
        assert torch.isfinite(got).all()
        err, bound = (got - refs[i]).abs().max().item(), 3e-5 * refs[i].abs().max().item()
        print(f"\n[g two problems L={L}] problem {i}: max err {err:.3e} (bound {bound:.3e})")
        assert err <= bound
