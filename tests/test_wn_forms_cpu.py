"""CPU: the references tests/test_wn_forms_gpu.py holds the fp32 WN layer's launches to.  (a) the packer's row permutation as the
library states it against its Python statement; (b) the per-launch restatements, chained, against the oracle's whole WN.forward in
fp64; (c) at the GPU tests' own inputs, every plausible kernel error moves the result by more than 100 bars, so the GPU bars cannot
pass it; (d) the launcher's gate refusals, which come from host-side checks alone."""
import ctypes as C

import pytest
import torch

from tests import wn_refs as R


def _lib():
    from bert_vits2_amd import lib as L
    lib = L.load()
    lib.bv2_test_wn_gate_row.restype = C.c_int
    lib.bv2_test_wn_gate_row.argtypes = [C.c_int, C.c_int]
    p = C.c_void_p
    lib.bv2_test_conv1d.restype = C.c_int
    lib.bv2_test_conv1d.argtypes = ([p] * 6 + [C.c_int] * 8 + [C.c_float, C.c_int, p, C.c_int, p, p, C.c_int, C.c_int, p, C.c_int, p, p,
                                    C.c_float, C.c_int, C.c_int64])
    return lib


# ---------------------------------------------------------------------------------------------------------------- (a)
@pytest.mark.parametrize("H", [32, 64, 128, 160, 192, 256])
def test_gate_row_is_the_python_statement_and_a_bijection(H):
    lib = _lib()
    rows = [lib.bv2_test_wn_gate_row(H, n) for n in range(2 * H)]
    assert rows == [R.gate_row(H, n) for n in range(2 * H)]
    assert sorted(rows) == list(range(2 * H))
    # what the kernels rely on: rows n and n + 16 of a 32-row tile are one channel's tanh and sigmoid rows, channels in natural order
    for n in range(0, 2 * H, 32):
        for j in range(16):
            assert rows[n + j] == n // 2 + j and rows[n + 16 + j] == H + n // 2 + j


def test_gate_orders_agree():
    B, H, L = 2, 64, 9
    v = torch.randn(B, 2 * H, L, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    assert torch.equal(R.gate_packed(v[:, R.gate_perm(H)]), R.gate(v, H))


# ---------------------------------------------------------------------------------------------------------------- (b)
def test_chained_restatements_are_the_oracles_wn():
    from oracle import bv2_oracle as O
    sd, x, gvec, mask = R.chain_inputs()
    B, H, L, _ = R.CHAIN_SHAPE
    sd64 = {k: v.double() for k, v in sd.items()}
    ref = O.wn(sd64, "wn", x.double(), mask.double()[:, None, :], gvec.double()[:, :, None], R.CHAIN_LAYERS, H)
    ins, rss = R.chain_layers(sd)
    gl_all = R.cond(gvec, sd["wn.cond_layer.weight"], sd["wn.cond_layer.bias"])
    steps = R.chain(x, gl_all, mask, ins, rss)
    err = (steps[-1]["out"] - ref).abs().max().item()
    print(f"\n[chain vs oracle.wn] max abs err {err:.3e} (scale {ref.abs().max().item():.3f})")
    assert ref.dtype == torch.float64 and err <= 1e-12
    assert mask[1, -1] == 0 and ref[1, :, -1].abs().max() == 0          # the ragged item really is masked
    # ... and the same chain on gate-order rows (what bv2_test_conv1d is given) gives the same activations
    perm = R.gate_perm(H)
    for i, s in enumerate(steps):
        w, b = ins[i]
        v = R.preact(s["x_in"], w[perm], b[perm], gl_all[:, 2 * H * i:2 * H * (i + 1)][:, perm])
        assert (R.gate_packed(v) - s["acts"]).abs().max().item() <= 1e-12


# ---------------------------------------------------------------------------------------------------------------- (c)
def _gate_gap(wrong, true, v):
    """in bars of the gate tests: |got - ref| <= BAR * max|v|"""
    return ((wrong - true).abs().max() / (R.BAR * v.abs().max())).item()


@pytest.mark.parametrize("B,H,L", sorted(set(R.GATE_TILE_SHAPES + R.GATE_SPLITK_SHAPES + R.IN_LAYER_SHAPES)))
def test_gate_inputs_discriminate(B, H, L):
    x, w, b, gl = R.in_inputs(B, H, L)
    v = R.preact(x, w, b, gl)
    true = R.gate(v, H)
    perm = R.gate_perm(H)
    vp = v[:, perm]
    gaps = {
        "halves swapped": _gate_gap(R.gate_halves_swapped(v, H), true, v),
        "halves swapped (gate order)": _gate_gap(R.gate_packed_halves_swapped(vp), true, v),
        "pairing (n, n+16) on reference-order rows": _gate_gap(R.gate_packed(v), true, v),
        "pairing (n, n+H) on gate-order rows": _gate_gap(R.gate(vp, H), true, v),
        "g_l unpermuted": _gate_gap(R.gate(R.preact(x, w, b, R.gl_unpermuted(gl, H)), H), true, v),
    }
    if B > 1:
        gaps["g_l of item 0 for every item"] = _gate_gap(R.gate(R.preact(x, w, b, R.gl_item0(gl)), H), true, v)
    print(f"\n[discrimination B={B} H={H} L={L}] " + ", ".join(f"{k}: {g:.0f} bars" for k, g in gaps.items()))
    for k, g in gaps.items():
        assert g > 100, k


@pytest.mark.parametrize("B,H,L,lens", R.RES_SKIP_SHAPES)
def test_res_skip_inputs_discriminate(B, H, L, lens):
    acts, w, b, x, outacc, mask = R.res_skip_inputs(B, H, L, lens)
    assert min(lens) < L                                               # padded columns exist: the order of add and mask shows
    gaps = {}
    for first, last, name in ((True, False, "first"), (False, False, "middle"), (False, True, "last")):
        ww, bb = (w[:H], b[:H]) if last else (w, b)
        xt, ot = R.res_skip(acts, ww, bb, x, outacc, mask, first, last)
        xw, ow = R.res_skip_add_after_mask(acts, ww, bb, x, outacc, mask, first, last)
        gaps[f"{name}: add after mask"] = R.rel_err(ow, ot) if last else R.rel_err(xw, xt)
        if not last:
            gaps[f"{name}: skip rows from [0,H)"] = R.rel_err(R.res_skip_rows_from_res(acts, ww, bb, x, outacc, mask, first), ot)
            assert all(xt[i, :, n:].abs().sum() == 0 for i, n in enumerate(lens))   # x is exactly 0 in the padded columns
    print(f"\n[discrimination res_skip B={B} H={H} L={L}] " + ", ".join(f"{k}: {g / R.BAR:.0f} bars" for k, g in gaps.items()))
    for k, g in gaps.items():
        assert g > 100 * R.BAR, k


# ---------------------------------------------------------------------------------------------------------------- (d)
def test_gate_refusals_come_before_any_device_call():
    """ACT_GATE with a K split, a residual, a mask, ragged tiles or an x6 / x3 tile: the -1 is launch_conv1d's, from its checks in front of
    any launch.  There is no device here and the pointers are not device memory: w_host = NULL and cin = 16 keep bv2_test_conv1d from
    packing, uploading or launching anything of its own on the way to the launcher.  (Without a device a launch would fail too: that the
    refusal launches nothing is what tests/test_wn_forms_gpu.py::test_gate_refusals_launch_nothing shows.)"""
    lib = _lib()
    buf = torch.zeros(64)
    p = C.c_void_p(buf.data_ptr())

    def call(tile=0, cout=64, res=None, res_mode=0, out_mask=None, mask_pre=0, mask_post=0, ksplit=1, act=2):
        return lib.bv2_test_conv1d(None, p, None, None, p, p, 1, 16, cout, 5, 1, -1, 8, tile, 0.0, act, res, res_mode, None, out_mask,
                                   mask_pre, mask_post, None, 1, None, None, 1.0, ksplit, 0)
    assert call(tile=6, ksplit=2) == -1
    assert call(res=p, res_mode=1) == -1 and call(res=p, res_mode=2) == -1
    assert call(out_mask=p) == -1 and call(mask_pre=1) == -1 and call(mask_post=1) == -1 and call(out_mask=p, mask_post=1) == -1
    assert call(cout=48) == -1 and call(cout=16) == -1
    for tile in (8, 9, 10, 11, 12, 14):
        assert call(tile=tile) == -1, tile
    assert call(act=4) == -1 and call(act=-1) == -1                    # no such activation
