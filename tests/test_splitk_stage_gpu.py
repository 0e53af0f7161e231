"""GPU: the split-K conv's block staging of its X tile (conv_mfma.hip, the head form: the workgroup's threads cover whole tile rows per
pass, a thread keeps one column), the text-encoder attention's key split at T = 128, and the x3 slots zeroed by phase B's front launch.

Staging.  The staged tile holds the same values at the same LDS addresses however it was filled, and the tap loop is untouched, so the
block-staged launch must be BITWISE equal to the row-per-wave staging (tuning 200 + waves) and to the register form (100 + waves), and
right against fp64 at the suite's fp32 bar (tests/test_kernels_gpu.py: 2e-5 of the output scale).  Shapes: every row-count class
(cin 8 / 40 / 192, and 200 < cin_pad), every tile width of k in {3, 5, 7} x dil in {1, 2} (34 / 36 / 38 / 44 columns), L with one-column,
ragged and several tiles (pad_left reaches before column 0 in each), K splits 1 / 2 / 8 on 4 and 8 waves, input mask on and off under a
leaky-ReLU pre-activation, B = 1 as the head form and as the generic kernel, B = 2 (generic).  Which staging a launch took is the
launcher's own report (bv2_test_splitk_stage), asserted where the test's purpose depends on it."""
import ctypes as C
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from oracle import cases
from tests import encoder_refs as R
from tests.helpers import cached_state_dict
from tests.test_encoder_forms_gpu import _case, _split_launch

pytestmark = pytest.mark.gpu

COUT = 40          # two row tiles, the second ragged
SLOPE = 0.1


@functools.lru_cache(maxsize=None)
def _lib():
    from bert_vits2_amd import lib as L
    lib = L.load()
    lib.bv2_test_conv_pack_floats.restype = C.c_int64
    lib.bv2_test_conv_pack_floats.argtypes = [C.c_int] * 3
    lib.bv2_test_conv1d.restype = C.c_int
    lib.bv2_test_conv1d.argtypes = ([C.c_void_p] * 6 + [C.c_int] * 8 + [C.c_float, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                    C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_float,
                                    C.c_int, C.c_int64])
    lib.bv2_test_set_tuning.argtypes = [C.c_int, C.c_int, C.c_long]
    lib.bv2_test_set_tuning.restype = None
    lib.bv2_test_set_kernarg_head.argtypes = [C.c_int]
    lib.bv2_test_set_kernarg_head.restype = None
    lib.bv2_test_splitk_stage.argtypes = []
    lib.bv2_test_splitk_stage.restype = C.c_int
    return lib


def P(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _launch(lib, tune, head, xd, md, w, bias, wp, B, cin, k, dil, L, ksplit):
    """One split-K launch (tile 6) under a tuning value; returns the summed slabs and the staging the launcher reports."""
    lib.bv2_test_set_tuning(tune, 0, 0)
    lib.bv2_test_set_kernarg_head(head)
    out = torch.full((ksplit, B, COUT, L), float("nan"), device="cuda")
    try:
        rc = lib.bv2_test_conv1d(None, P(xd), P(w), P(bias), P(out), P(wp), B, cin, COUT, k, dil, -1, L, 6, SLOPE, 0, None, 0,
                                 P(md), None, 0, 0, None, 1, None, None, 1.0, ksplit, B * COUT * L)
        stage = lib.bv2_test_splitk_stage()
        torch.cuda.synchronize()
    finally:
        lib.bv2_test_set_tuning(0, 0, 0)
        lib.bv2_test_set_kernarg_head(1)
    assert rc == 0
    return out.sum(0).cpu(), stage


def _expected_stage(cin, k, dil, waves, ksplit):
    """The launcher's rule, restated: rows of the largest slice, whole rows per pass, the instantiation that covers them."""
    groups = (cin + 15) // 16 * 2
    nsl = ksplit * waves
    rows = max(8 * (groups * (z + 1) * waves // nsl - groups * z * waves // nsl) for z in range(ksplit))
    if rows > 32 * waves:
        return -1                                   # the tile does not fit: register form
    need = -(-rows // (64 * waves // (32 + (k - 1) * dil)))
    return 16 if need <= 16 else (24 if need <= 24 else 0)


def _check(cin, k, dil, waves, ksplit, Ls=(1, 31, 33, 70)):
    lib = _lib()
    g = torch.Generator().manual_seed(1000 * cin + 10 * k + dil)
    w = torch.randn(COUT, cin, k, generator=g) / math.sqrt(cin * k)
    bias = torch.randn(COUT, generator=g)
    wp = torch.empty(lib.bv2_test_conv_pack_floats(cin, COUT, k), device="cuda")
    want = _expected_stage(cin, k, dil, waves, ksplit)
    seen = set()
    for L in Ls:
        for B, head, masked in ((1, 1, True), (1, 1, False), (1, 0, True), (2, 1, True), (2, 1, False)):
            x = torch.randn(B, cin, L, generator=g)
            mask = (torch.arange(L)[None, :] < torch.tensor([L, max(1, L - 9)][:B])[:, None]).float()
            if B == 1 and masked and L > 4:
                mask[0, L - 3:] = 0.0               # a masked tail at B = 1 too
            xd, md = x.cuda(), (mask.cuda() if masked else None)
            new, st_new = _launch(lib, waves, head, xd, md, w, bias, wp, B, cin, k, dil, L, ksplit)
            row, st_row = _launch(lib, 200 + waves, head, xd, md, w, bias, wp, B, cin, k, dil, L, ksplit)
            reg, st_reg = _launch(lib, 100 + waves, head, xd, md, w, bias, wp, B, cin, k, dil, L, ksplit)
            tag = f"cin={cin} k={k} dil={dil} waves={waves} ksplit={ksplit} L={L} B={B} head={head} mask={masked}"
            assert st_reg == -1 and st_row == (0 if want >= 0 else -1), (tag, st_row, st_reg)
            assert st_new == (want if (B == 1 and head) else min(want, 0)), (tag, st_new, want)
            seen.add(st_new)
            assert torch.equal(new, row), tag
            assert torch.equal(new, reg), tag
            xin = F.leaky_relu(x.double(), SLOPE) * (mask.double()[:, None] if masked else 1.0)
            ref = F.conv1d(xin, w.double(), bias.double(), padding=(k - 1) // 2 * dil, dilation=dil)
            err = ((new.double() - ref).abs().max() / ref.abs().max().clamp_min(1e-30)).item()
            assert err < 2e-5, (tag, err)
    return seen


@pytest.mark.parametrize("k,dil", [(3, 1), (5, 1), (7, 1), (7, 2)])
@pytest.mark.parametrize("cin", [8, 40, 192, 200])
def test_block_staging_is_bit_identical_to_row_staging_and_register_form(cin, k, dil):
    seen = set()
    for waves in (4, 8):
        for ksplit in (1, 2, 8):
            seen |= _check(cin, k, dil, waves, ksplit)
    print(f"\n[cin={cin} k={k} dil={dil}] stagings taken: {sorted(seen)}")
    assert 16 in seen                                  # every (cin, tile width) has splits whose tile fits 16 loads per thread
    if cin == 200 and (k, dil) == (7, 2):
        assert 24 in seen                              # 208 rows x 44 columns on 8 waves: 19 per thread


def test_block_staging_falls_back_past_the_largest_instantiation():
    """128 rows x 50 columns (k = 7, dil = 3) on 4 waves: 5 whole rows per pass, 26 loads per thread > 24 — the head form keeps the
    row-per-wave staging, same bits."""
    assert _expected_stage(128, 7, 3, 4, 1) == 0
    seen = _check(128, 7, 3, 4, 1, Ls=(33, 70))
    assert 0 in seen and 16 not in seen and 24 not in seen


# ------------------------------------------------------------------------------------------------------------------
# attention: the key split at T = 97 / 128 (four key tiles), both splits against fp64 at the bars of tests/test_kernels_gpu.py /
# test_encoder_forms_gpu.py (2e-5 of the output scale)

@pytest.mark.parametrize("ks", [1, 2])
@pytest.mark.parametrize("T", [97, 128])
def test_attention_two_key_ranges_at_four_tiles(T, ks):
    B, H, D, Co, lens = 1, 2, 96, 192, (T,)
    if ks == 1:
        from tests.test_encoder_forms_gpu import _launch_fused
        c = _case(B, T, lens, H, D, 3.0)
        wo, bo, res = R.conv_o_weights(H, D, Co, B, T)
        rc, slabs, _ = _launch_fused(c, B, T, H, D, Co, wo, bo, res)
        assert rc == 0
        got = slabs.sum(0)
    else:
        c, wo, bo, res, slabs, ml = _split_launch(B, T, lens, H, D, ks, 3.0, Co)
        got = R.ref_split_merge(slabs, ml[:, :, :, 0], ml[:, :, :, 1]) + bo.double()[None, :, None] + res.double()
    ref = R.ref_conv_o(c["att"], wo, bo, res)
    assert torch.isfinite(got).all()
    err, bound = (got - ref).abs().max().item(), 2e-5 * ref.abs().max().item()
    print(f"\n[T={T} ks={ks}] max err {err:.3e} (bound {bound:.3e})")
    assert err <= bound


# ------------------------------------------------------------------------------------------------------------------
# x3 slots: zeroed by phase B's front launch, every decode — eager and replayed

def test_repeated_decodes_eager_and_replayed_are_identical_and_finite():
    """The fp32 Generator's max-|x| slots are max-accumulated by their publishers, so a decode that starts from the previous one's
    values scales its fp16 planes wrongly (a NaN on the second graph replay was the first sign).  Same B = 1 inputs three times
    eagerly, three times replayed: one waveform."""
    from bert_vits2_amd import models
    hp, seed, batch, nw, nz, kw = cases.build_case("zh_b1_t24")
    m = models.from_hparams(hp)
    m.load_state_dict(cached_state_dict(hp, seed), strict=False)
    m = m.to("cuda").eval()
    args = [batch[k].cuda() for k in ("x", "x_lengths", "sid", "tone", "language", "bert", "ja_bert", "en_bert")]

    def run():
        o = m.infer(*args, noise_w=nw.cuda(), noise_z=nz.cuda(), **kw)[0]
        torch.cuda.synchronize()
        return o.clone()

    eager = [run() for _ in range(3)]
    m.enable_graphs(True, ty_bucket=1)
    replayed = [run() for _ in range(3)]
    m.enable_graphs(False)
    assert len(eager[0].shape) == 3 and torch.isfinite(eager[0]).all()
    for o in eager[1:] + replayed:
        assert torch.equal(o, eager[0])
