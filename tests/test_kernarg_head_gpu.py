"""GPU: the head forms of the batch-1 launch chain (bv2_set_option("kernarg_head"), bv2_kernels.h SkHead) against the generic kernels
they stand in for, inside one build.  A head kernel receives what a workgroup needs for its first global loads as leading scalar
arguments (preloaded into SGPRs) and the rest in the argument struct; arithmetic, summation order and tile shapes are the generic
kernel's, so every output must be BIT-identical: each case launches the same inputs with the switch at 0 and at 1 and compares the two
output buffers as integers (NaN guards around the written region included, so a stray store shows too).

Shapes are the smallest at which the forms differ in path: the non-staged (k = 1) and the LDS-staged (k > 1) split-K forms, a partial
last column tile (T = 37) and several tiles (T = 96), one slab and eight, C_in off the padding (100 of 112 rows), and launches that must
fall back (B = 2 with `lens`; a dilation that does not fit its 8-bit field)."""
import ctypes as C
import functools
import math

import pytest
import torch

from tests import encoder_refs as R
from tests import test_attention_qtile_gpu as Q
from tests import test_encoder_forms_gpu as F

pytestmark = pytest.mark.gpu


def P(t):
    return None if t is None else C.c_void_p(t.data_ptr())


class Prob(C.Structure):                                           # bv2_testing.h bv2_test_conv_prob
    _fields_ = [("w_host", C.c_void_p), ("bias_host", C.c_void_p), ("k", C.c_int32), ("dil", C.c_int32), ("pad_left", C.c_int32),
                ("out", C.c_void_p), ("out_rstride", C.c_int32), ("out_tstride", C.c_int32), ("out_toff", C.c_int32),
                ("res", C.c_void_p), ("res_mode", C.c_int32)]


@functools.lru_cache(maxsize=None)
def _lib():
    lib = Q._lib()
    p, i, i64, f = C.c_void_p, C.c_int, C.c_int64, C.c_float
    lib.bv2_test_set_kernarg_head.restype = None
    lib.bv2_test_set_kernarg_head.argtypes = [i]
    lib.bv2_test_conv_pack_floats.restype = i64
    lib.bv2_test_conv_pack_floats.argtypes = [i] * 3
    lib.bv2_test_conv1d.restype = i
    lib.bv2_test_conv1d.argtypes = [p] * 6 + [i] * 8 + [f, i, p, i, p, p, i, i, p, i, p, p, f, i, i64]
    lib.bv2_test_conv_multi_pack_floats.restype = i64
    lib.bv2_test_conv_multi_pack_floats.argtypes = [i, i, p, i]
    lib.bv2_test_conv_multi.restype = i
    lib.bv2_test_conv_multi.argtypes = [p, p, i, i, i, p, p, p, i, f, f, p, i, i, i, i, i, i64, p, p, p, p]
    return lib


def both_forms(launch):
    """launch() -> tensor of everything the launch wrote, once per form; asserts the two are the same bits."""
    lib = _lib()
    got = []
    try:
        for on in (0, 1):
            lib.bv2_test_set_kernarg_head(on)
            got.append(launch())
            torch.cuda.synchronize()
    finally:
        lib.bv2_test_set_kernarg_head(1)
    a, b = (t.contiguous().view(torch.int32) for t in got)
    assert torch.equal(a, b), f"{(a != b).sum().item()} of {a.numel()} words differ between kernarg_head 0 and 1"
    return got[1]


# ------------------------------------------------------------------------------------------------------------------
# split-K

@pytest.mark.parametrize("T", [37, 96])
@pytest.mark.parametrize("ksplit", [1, 8])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("cin,cout,k", [(192, 64, 1), (192, 64, 5), (256, 32, 3)])
def test_splitk_head_equals_generic(cin, cout, k, masked, ksplit, T):
    lib = _lib()
    g = torch.Generator().manual_seed(cin + 7 * k + T)
    x = torch.randn(1, cin, T, generator=g).cuda()
    w = torch.randn(cout, cin, k, generator=g) / math.sqrt(cin * k)
    bias, res = torch.randn(cout, generator=g), torch.randn(1, cout, T, generator=g).cuda()
    mask = (torch.arange(T)[None, :] < T - 5).float().cuda() if masked else None
    wp = torch.empty(lib.bv2_test_conv_pack_floats(cin, cout, k), device="cuda")

    def launch():
        out = torch.full((ksplit + 1, 1, cout, T), float("nan"), device="cuda")     # one guard slab behind the last
        rc = lib.bv2_test_conv1d(None, P(x), P(w), P(bias), P(out), P(wp), 1, cin, cout, k, 1, -1, T, 6, 0.1, 0, P(res), 1,
                                 P(mask), P(mask), 1 if masked else 0, 0, None, 1, None, None, 0.5, ksplit, cout * T)
        assert rc == 0
        return out
    out = both_forms(launch)
    assert torch.isfinite(out[:ksplit]).all() and torch.isnan(out[ksplit]).all()
    # and the head form computes the conv (fp32 round-off of a sum of cin * k products): not merely the same as the other form
    xin = torch.nn.functional.leaky_relu(x.double().cpu() * 0.5, 0.1) * (1 if mask is None else mask.double().cpu()[:, None])
    ref = torch.nn.functional.conv1d(xin, w.double(), bias.double(), padding=(k - 1) // 2)
    if masked:
        ref = ref * mask.double().cpu()[:, None]
    ref = ref + res.double().cpu()
    err = (out[:ksplit].sum(0).double().cpu() - ref).abs().max().item()
    print(f"\n[split-K {cin}->{cout} k={k} T={T} ks={ksplit} mask={masked}] max err {err:.3e} at scale {ref.abs().max().item():.3e}")
    assert err <= 2e-5 * ref.abs().max().item()


def test_splitk_head_ragged_channels():
    """C_in = 100 (cin_pad 112): the last channel group is clamped to the last real row and meets zero weights."""
    lib = _lib()
    cin, cout, k, T = 100, 64, 5, 37
    g = torch.Generator().manual_seed(100)
    x = torch.randn(1, cin, T, generator=g).cuda()
    w = torch.randn(cout, cin, k, generator=g) / math.sqrt(cin * k)
    bias = torch.randn(cout, generator=g)
    mask = (torch.arange(T)[None, :] < T - 5).float().cuda()
    wp = torch.empty(lib.bv2_test_conv_pack_floats(cin, cout, k), device="cuda")

    def launch():
        out = torch.full((2, 1, cout, T), float("nan"), device="cuda")
        assert lib.bv2_test_conv1d(None, P(x), P(w), P(bias), P(out), P(wp), 1, cin, cout, k, 1, -1, T, 6, 0.0, 0, None, 0,
                                   P(mask), P(mask), 0, 1, None, 1, None, None, 1.0, 1, 0) == 0
        return out
    out = both_forms(launch)
    ref = torch.nn.functional.conv1d(x.double().cpu() * mask.double().cpu()[:, None], w.double(), bias.double(), padding=2) * mask.double().cpu()[:, None]
    assert torch.isnan(out[1]).all()
    assert (out[0].double().cpu() - ref).abs().max().item() <= 2e-5 * ref.abs().max().item()


def test_splitk_batch_with_lens_takes_the_generic_form():
    """B = 2 with exact lengths: the clamp of Lin needs a load first, so the launcher keeps the generic kernel whatever the switch says."""
    lib = _lib()
    B, cin, cout, k, T = 2, 192, 64, 5, 37
    g = torch.Generator().manual_seed(5)
    x = torch.randn(B, cin, T, generator=g).cuda()
    w = (torch.randn(cout, cin, k, generator=g) / math.sqrt(cin * k)).contiguous()
    bias = torch.randn(cout, generator=g)
    lens = torch.tensor([T, 20], dtype=torch.int64).cuda()
    kt = torch.tensor([k], dtype=torch.int32)
    wp = torch.empty(lib.bv2_test_conv_multi_pack_floats(cin, cout, P(kt), 1), device="cuda")

    def launch():
        out = torch.full((2, B, cout, T), float("nan"), device="cuda")
        probs = (Prob * 1)(Prob(w.data_ptr(), bias.data_ptr(), k, 1, -1, out.data_ptr(), T, 1, 0, None, 0))
        assert lib.bv2_test_conv_multi(None, probs, 1, cin, cout, P(x), None, None, 1, 1.0, 0.0, P(lens), 1, B, T, 6, 1, B * cout * T,
                                       None, None, P(wp), None) == 0
        return out
    out = both_forms(launch)
    xz = x.double().cpu().clone()
    xz[1, :, 20:] = 0                                              # positions past an item's length read as the conv's zero padding
    ref = torch.nn.functional.conv1d(xz, w.double(), bias.double(), padding=2)
    assert torch.isnan(out[1]).all()
    assert (out[0].double().cpu() - ref).abs().max().item() <= 2e-5 * ref.abs().max().item()


def test_splitk_wide_dilation_falls_back():
    """dil = 256 does not fit the head's 8-bit field (nor does its pad_left): the generic kernel runs, and the result is the conv."""
    lib = _lib()
    cin, cout, k, dil, T = 192, 64, 3, 256, 300
    g = torch.Generator().manual_seed(256)
    x = torch.randn(1, cin, T, generator=g).cuda()
    w = torch.randn(cout, cin, k, generator=g) / math.sqrt(cin * k)
    bias = torch.randn(cout, generator=g)
    wp = torch.empty(lib.bv2_test_conv_pack_floats(cin, cout, k), device="cuda")

    def launch():
        out = torch.full((2, 1, cout, T), float("nan"), device="cuda")
        assert lib.bv2_test_conv1d(None, P(x), P(w), P(bias), P(out), P(wp), 1, cin, cout, k, dil, -1, T, 6, 0.0, 0, None, 0,
                                   None, None, 0, 0, None, 1, None, None, 1.0, 1, 0) == 0
        return out
    out = both_forms(launch)
    ref = torch.nn.functional.conv1d(x.double().cpu(), w.double(), bias.double(), padding=dil, dilation=dil)
    assert torch.isnan(out[1]).all()
    assert (out[0].double().cpu() - ref).abs().max().item() <= 2e-5 * ref.abs().max().item()


# ------------------------------------------------------------------------------------------------------------------
# LayerNorm

@pytest.mark.parametrize("T", [9, 40])
@pytest.mark.parametrize("Cc", [192, 256])
@pytest.mark.parametrize("nslab", [1, 8])
def test_layernorm_head_equals_generic(nslab, Cc, T):
    """Slab sum + residual, with the speaker vector and the mask in the epilogue.  B = 1: the head forms are batch-1 forms."""
    B = 1
    g = torch.Generator().manual_seed(nslab + Cc + T)
    a = torch.randn(nslab, B, Cc, T, generator=g).cuda()
    add, vec = torch.randn(B, Cc, T, generator=g).cuda(), torch.randn(B, Cc, generator=g).cuda()
    gamma, beta = torch.randn(Cc, generator=g).cuda(), torch.randn(Cc, generator=g).cuda()
    mask = F.len_mask([max(1, T - 4)], T).cuda()

    def launch():
        out = F.nanf(2, B, Cc, T)
        assert F.layernorm_ex(a=a, add=add, gamma=gamma, beta=beta, vec=vec, mask=mask, out=out, B=B, C=Cc, T=T, nslab=nslab,
                              slab_stride=B * Cc * T) == 0
        return out
    out = both_forms(launch)
    v = a.double().sum(0) + add.double()
    ref = (torch.nn.functional.layer_norm(v.transpose(1, 2), (Cc,), gamma.double(), beta.double(), 1e-5).transpose(1, 2)
           + vec.double()[:, :, None]) * mask.double()[:, None]
    assert torch.isnan(out[1]).all()
    err = (out[0].double() - ref).abs().max().item()
    print(f"\n[LayerNorm nslab={nslab} C={Cc} T={T}] max err {err:.3e}")
    assert err <= 1e-5 * max(ref.abs().max().item(), 1.0) * math.sqrt(nslab)


@pytest.mark.parametrize("T", [9, 40])
def test_layernorm_weighted_slabs_head_equals_generic(T):
    """The key-split merge: two heads x four key ranges (KS = 4), conv_o's bias and the residual."""
    B, Cc, Hh, ks = 1, 192, 2, 4
    g = torch.Generator().manual_seed(T)
    a = torch.randn(Hh * ks, B, Cc, T, generator=g).cuda()
    ml = torch.randn(B, Hh, ks, 2, T, generator=g)
    ml[:, :, :, 1] = ml[:, :, :, 1].abs() + 0.5                    # the ranges' softmax sums are positive
    ml = ml.cuda()
    add, bias = torch.randn(B, Cc, T, generator=g).cuda(), torch.randn(Cc, generator=g).cuda()
    gamma, beta = torch.randn(Cc, generator=g).cuda(), torch.randn(Cc, generator=g).cuda()

    def launch():
        out = F.nanf(2, B, Cc, T)
        assert F.layernorm_ex(a=a, add=add, gamma=gamma, beta=beta, out=out, B=B, C=Cc, T=T, nslab=Hh * ks, slab_stride=B * Cc * T,
                              ml=ml, ml_H=Hh, ml_ks=ks, bias=bias) == 0
        return out
    out = both_forms(launch)
    m, l = ml[:, :, :, 0].double(), ml[:, :, :, 1].double()
    wgt = l * torch.exp(m - m.max(2, keepdim=True).values)
    wgt = wgt / wgt.sum(2, keepdim=True)                           # [B][H][ks][T]
    v = (a.double().view(Hh, ks, B, Cc, T) * wgt.permute(1, 2, 0, 3)[:, :, :, None, :]).sum((0, 1)) + bias.double()[None, :, None] + add.double()
    ref = torch.nn.functional.layer_norm(v.transpose(1, 2), (Cc,), gamma.double(), beta.double(), 1e-5).transpose(1, 2)
    assert torch.isnan(out[1]).all()
    err = (out[0].double() - ref).abs().max().item()
    print(f"\n[LayerNorm weighted slabs T={T}] max err {err:.3e}")
    assert err <= 1e-5 * max(ref.abs().max().item(), 1.0) * math.sqrt(Hh * ks)


# ------------------------------------------------------------------------------------------------------------------
# attention, fp32 with the fused conv_o: head dim 96, two heads

@pytest.mark.parametrize("T,ks", [(33, 1), (130, 1), (130, 2), (130, 4)])
def test_attention_head_equals_generic(T, ks):
    """T = 33: 16-query tiles, no key split.  T = 130 (five key tiles): attention_pick_ksplit keeps one range below nine key tiles, so
    both split forms are forced beside it (two heads x 2 / 4 ranges = 4 / 8 slabs)."""
    B, H, D, Co = 1, 2, 96, 192
    c = F._case(B, T, (T,), H, D, 3.0)
    wo, bo, res = R.conv_o_weights(H, D, Co, B, T)
    if ks > 1:
        bo = res = None                                            # the key split carries neither: the LayerNorm adds them
    ref = R.ref_conv_o(c["att"], wo, bo, res)

    def launch():
        rc, slabs, ml = Q._launch_fused(c, B, T, H, D, Co, wo, 0, bo, res, ks)
        assert rc == 0
        return slabs.float() if ml is None else torch.cat([slabs.float().flatten(), ml.float().flatten()])
    out = both_forms(launch)
    assert torch.isfinite(out).all()
    if ks == 1:
        err = (out.double().sum(0) - ref).abs().max().item()
        print(f"\n[attention T={T}] slab sum: max err {err:.3e}")
        assert err <= 2e-5 * ref.abs().max().item()


# ------------------------------------------------------------------------------------------------------------------
# flow boundary: the smallest case of tests/test_flow_boundary_gpu.py (B = 3: every launch keeps its generic kernel, whatever the switch says)
# and the same at B = 1, where every launch of the flow takes its head form or not; through the model

@pytest.mark.parametrize("B,Ty,lens", [(3, 9, [9, 1, 4]), (1, 9, [9])])
def test_flow_with_heads_equals_generic(B, Ty, lens):
    from oracle import cases
    from tests.test_flow_boundary_gpu import _gpu_model
    hp, seed, *_ = cases.build_case("zh_b1_t24")
    m = _gpu_model(hp, seed)
    gen = torch.Generator().manual_seed(Ty + B)
    z_p = torch.randn(B, hp.inter_channels, Ty, generator=gen).cuda()
    g = torch.randn(B, hp.gin_channels, 1, generator=gen).cuda()
    yl = torch.tensor(lens, dtype=torch.int64).cuda()
    m.set_option("fused_boundary", 1)
    m.set_option("kernarg_head", 0)
    z0 = m.stage_flow(z_p, yl, g).clone()
    m.set_option("kernarg_head", 1)
    z1 = m.stage_flow(z_p, yl, g).clone()
    torch.cuda.synchronize()
    assert torch.isfinite(z1).all()
    assert torch.equal(z0, z1)
