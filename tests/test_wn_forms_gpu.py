"""GPU: the fp32 WaveNet layer's two launches (bv2_exec.cpp run_wn) at kernel level against the fp64 restatements of tests/wn_refs.py:
the ACT_GATE epilogue of the tile kernel at every tile and of the split-K kernel in its 8- and 4-wave, head and generic forms
(kernels/conv_mfma.hip), in_layer from reference-order weights through the packer's permutation, the res_skip launch in its first,
middle and last forms at every tile, one layer at a time on teacher-forced inputs, and the launcher's gate refusals.

Bars.  Gate: elementwise |got - ref| <= 2e-5 * max|v|, v = conv + bias + g_l in fp64: 2e-5 of the output scale is the bar
test_conv1d_mfma_plain holds this kernel's accumulator to, the gate's slope in v is at most 1, and fp32 tanhf / expf add a few ulp of a
value <= 1 (1e-7, no term).  res_skip: rel_err < 2e-5 per output tensor, padded columns included (test_conv1d_splitk_fused_epilogues'
bar).  tests/test_wn_forms_cpu.py shows that each plausible kernel error misses these by more than 100 bars at these inputs.

Every output buffer is NaN before its launch (the in-place ones hold their residual); the gate output has a guard block of 32 rows
behind the last item's last row — items are cout / 2 rows apart, so a row written past an earlier item's last lands in the next
item and shows as a wrong value — which must stay NaN.  (What this cannot show: a stray write into the next item's rows that the
workgroup owning them overwrites afterwards with the right value.)  Every test prints its figure (largest err / bar) before it asserts."""
import ctypes as C

import pytest
import torch

from tests import wn_refs as R

pytestmark = pytest.mark.gpu

K, BAR, GUARD = R.K, R.BAR, 32


def _lib():
    from bert_vits2_amd import lib as L
    lib = L.load()
    p, i, f, i64 = C.c_void_p, C.c_int, C.c_float, C.c_int64
    lib.bv2_test_conv_pack_floats.restype = i64
    lib.bv2_test_conv_pack_floats.argtypes = [i] * 3
    lib.bv2_test_conv1d.restype = i
    lib.bv2_test_conv1d.argtypes = [p] * 6 + [i] * 8 + [f, i, p, i, p, p, i, i, p, i, p, p, f, i, i64]
    lib.bv2_test_wn_in_pack_floats.restype = i64
    lib.bv2_test_wn_in_pack_floats.argtypes = [i, i]
    lib.bv2_test_wn_in_layer.restype = i
    lib.bv2_test_wn_in_layer.argtypes = [p] * 7 + [i] * 4
    lib.bv2_test_wn_res_skip_pack_floats.restype = i64
    lib.bv2_test_wn_res_skip_pack_floats.argtypes = [i]
    lib.bv2_test_wn_res_skip.restype = i
    lib.bv2_test_wn_res_skip.argtypes = [p] * 8 + [i] * 6
    lib.bv2_test_set_kernarg_head.restype = None
    lib.bv2_test_set_kernarg_head.argtypes = [i]
    lib.bv2_test_splitk_stage.restype = i
    lib.bv2_test_splitk_stage.argtypes = []
    lib.bv2_test_splitk_waves.restype = i
    lib.bv2_test_splitk_waves.argtypes = []
    return lib


def P(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def nan(*shape):
    return torch.full(shape, float("nan"), device="cuda")


# ---------------------------------------------------------------------------------------------------------------- launches
def gate_conv1d(lib, x, w, b, gl, tile, **kw):
    """bv2_test_conv1d with ACT_GATE on rows as given (gate order).  Returns (status, the whole [B * H + GUARD][L] output buffer)."""
    B, H, L = x.shape
    cout = w.shape[0]
    out = nan(B * (cout // 2) + GUARD, L)
    wp = torch.empty(lib.bv2_test_conv_pack_floats(H, cout, K), device="cuda")
    xd, gd, w, b = x.cuda(), gl.cuda().contiguous(), w.contiguous(), b.contiguous()
    res, om = kw.get("res"), kw.get("out_mask")
    rc = lib.bv2_test_conv1d(None, P(xd), P(w), P(b), P(out), P(wp), B, H, cout, K, 1, -1, L, tile, 0.0, 2,
                             P(res), kw.get("res_mode", 0), None, P(om), kw.get("mask_pre", 0), kw.get("mask_post", 0), P(gd), 1, None, None,
                             1.0, kw.get("ksplit", 1), kw.get("slab_stride", 0))
    torch.cuda.synchronize()
    return rc, out.cpu()


def wn_in_layer(lib, x, w, b, gl, tile, xd=None, acts=None):
    B, H, L = x.shape
    acts = nan(B * H + GUARD, L) if acts is None else acts
    wp = torch.empty(lib.bv2_test_wn_in_pack_floats(B, H), device="cuda")
    xd = x.cuda() if xd is None else xd
    w, b, gl = w.contiguous(), b.contiguous(), gl.contiguous()         # (held here: a slice's contiguous copy must outlive the call)
    rc = lib.bv2_test_wn_in_layer(None, P(xd), P(w), P(b), P(gl), P(acts), P(wp), B, H, L, tile)
    torch.cuda.synchronize()
    return rc, acts


def wn_res_skip(lib, acts_d, w, b, x_d, out_d, mask_d, tile, first, last):
    B, H, L = x_d.shape
    wp = torch.empty(lib.bv2_test_wn_res_skip_pack_floats(H), device="cuda")
    w, b = w.contiguous(), b.contiguous()
    rc = lib.bv2_test_wn_res_skip(None, P(acts_d), P(w), P(b), P(x_d), P(out_d), P(mask_d), P(wp), B, H, L, tile, int(first), int(last))
    torch.cuda.synchronize()
    return rc


def check_gate(tag, buf, ref, v):
    """buf: the whole output buffer (CPU); ref [B][H][L], v the fp64 pre-activation.  Returns the largest err / bar."""
    B, H, L = ref.shape
    got = buf[:B * H].reshape(B, H, L).double()
    worst = ((got - ref).abs().max() / (BAR * v.abs().max())).item()
    print(f"\n[{tag}] largest err / bar {worst:.4f} (max|v| {v.abs().max().item():.2f})")
    assert torch.isnan(buf[B * H:]).all(), "a row past cout / 2 of the last item was written"
    assert torch.isfinite(got).all()
    assert worst <= 1.0
    return worst


# ---------------------------------------------------------------------------------------------------------------- the gate epilogues
@pytest.mark.parametrize("tile", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("B,H,L", R.GATE_TILE_SHAPES)
def test_gate_tile_kernel(B, H, L, tile):
    """rows r and r + 8 of a lane as a (tanh, sigmoid) pair, stored at (row0 - 4 lh) / 2 + 4 lh: every tile shape, a ragged last 32-column
    block (77), a 128- and a 256-column tile edge (300), distinct g_l per item."""
    lib = _lib()
    x, w, b, gl = R.in_inputs(B, H, L)
    perm = R.gate_perm(H)
    wg, bg, glg = w[perm], b[perm], gl[:, perm]
    v = R.preact(x, wg, bg, glg)
    rc, buf = gate_conv1d(lib, x, wg, bg, glg, tile)
    assert rc == 0
    check_gate(f"gate tile {tile} B={B} H={H} L={L}", buf, R.gate_packed(v), v)


@pytest.mark.parametrize("B,H,L", R.GATE_SPLITK_SHAPES)
def test_gate_splitk_kernel(B, H, L):
    """pass i with pass i + 16 / RPP of one thread, stored at m0 / 2 + rl: the 8-wave form (H = 192: 120 units, 8 slices) and the 4-wave form
    (H = 64: 40 units, 3 slices), each in the batch-1 head form and in the generic form (B = 2); the head form bit for bit with the head off."""
    lib = _lib()
    x, w, b, gl = R.in_inputs(B, H, L)
    perm = R.gate_perm(H)
    wg, bg, glg = w[perm], b[perm], gl[:, perm]
    v = R.preact(x, wg, bg, glg)
    rc, buf = gate_conv1d(lib, x, wg, bg, glg, 6)
    stage, waves = lib.bv2_test_splitk_stage(), lib.bv2_test_splitk_waves()
    assert rc == 0
    print(f"\n[gate split-K B={B} H={H} L={L}] staging {stage}, {waves} waves")
    assert waves == (8 if H == 192 else 4), "the other instantiation's gate epilogue (RPP = 2 * waves) ran"
    assert stage >= 0, "the staged (LDSX) form is the only one a k = 5 in_layer reaches"
    if B == 1:
        assert stage in (16, 24), "the head form stages by blocks"
    check_gate(f"gate split-K B={B} H={H} L={L}", buf, R.gate_packed(v), v)
    if B == 1:
        lib.bv2_test_set_kernarg_head(0)
        try:
            rc2, buf2 = gate_conv1d(lib, x, wg, bg, glg, 6)
            stage2, waves2 = lib.bv2_test_splitk_stage(), lib.bv2_test_splitk_waves()
        finally:
            lib.bv2_test_set_kernarg_head(1)
        assert rc2 == 0 and stage2 == 0 and waves2 == waves            # the generic kernel: staged, a row per wave
        n = B * H
        assert torch.equal(buf[:n], buf2[:n]) and torch.isnan(buf2[n:]).all()


@pytest.mark.parametrize("B,H,L", R.IN_LAYER_SHAPES)
def test_in_layer_from_reference_order(B, H, L):
    """bv2_test_wn_in_layer permutes weight, bias and g_l with the packer's wn_gate_row: against the gate on reference-order rows, and bit
    for bit the bv2_test_conv1d run on rows permuted in Python — the packer's permutation is the kernel's pairing."""
    lib = _lib()
    x, w, b, gl = R.in_inputs(B, H, L)
    v = R.preact(x, w, b, gl)
    rc, acts = wn_in_layer(lib, x, w, b, gl, 0)
    assert rc == 0
    buf = acts.cpu()
    check_gate(f"in_layer B={B} H={H} L={L}", buf, R.gate(v, H), v)
    perm = R.gate_perm(H)
    rc2, buf2 = gate_conv1d(lib, x, w[perm], b[perm], gl[:, perm], 0)
    assert rc2 == 0
    assert torch.equal(buf[:B * H], buf2[:B * H])


# ---------------------------------------------------------------------------------------------------------------- res_skip
FORMS = {"first": (True, False), "middle": (False, False), "last": (False, True)}


def check_res_skip(tag, lib, acts, w, b, x, outacc, mask, tile, first, last):
    """One res_skip launch on fp32 inputs (CPU tensors, left unchanged) against the restatement on the same values.  x and outacc are
    their own residuals, as in run_wn; with `first` outacc starts as NaN.  Returns (largest rel_err / bar, x after, outacc after)."""
    H = acts.shape[1]
    ww, bb = (w[:H], b[:H]) if last and w.shape[0] == 2 * H else (w, b)
    x_ref, o_ref = R.res_skip(acts, ww, bb, x, outacc, mask, first, last)
    ad, xd, md = acts.cuda(), x.clone().cuda(), mask.cuda()
    od = nan(*x.shape) if first else outacc.clone().cuda()
    rc = wn_res_skip(lib, ad, ww, bb, xd, od, md, tile, first, last)
    assert rc == 0
    xg, og = xd.cpu(), od.cpu()
    ex, eo = R.rel_err(xg, x_ref), R.rel_err(og, o_ref)
    print(f"\n[{tag}] rel_err / bar: x {ex / BAR:.4f}, outacc {eo / BAR:.4f}")
    assert torch.isfinite(og).all(), "outacc has a NaN left"
    if last:
        assert torch.equal(xg, x)                                      # the last layer leaves x alone
    else:
        assert bool((xg[(mask == 0)[:, None, :].expand_as(xg)] == 0).all()), "x is not exactly 0 in the padded columns"
    assert ex < BAR and eo < BAR
    return max(ex, eo) / BAR, xg, og


@pytest.mark.parametrize("tile", [0, 1, 2, 3, 4, 5, 6])
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("B,H,L,lens", R.RES_SKIP_SHAPES)
def test_res_skip_launch(B, H, L, lens, form, tile):
    """Problem 0: rows [0,H), x = (x + rs) * mask in place.  Problem 1: rows [H,2H) into outacc, added unless first, never masked.  Last
    layer: one problem of H rows into outacc, masked."""
    lib = _lib()
    acts, w, b, x, outacc, mask = R.res_skip_inputs(B, H, L, lens)
    first, last = FORMS[form]
    check_res_skip(f"res_skip {form} tile {tile} B={B} H={H} L={L}", lib, acts, w, b, x, outacc, mask, tile, first, last)


# ---------------------------------------------------------------------------------------------------------------- one layer at a time
def test_layers_teacher_forced_and_chained():
    """Three layers of an fp64 WN (tests/test_wn_forms_cpu.py: it is the oracle's).  Teacher-forced: each launch runs on its fp64 inputs
    rounded to fp32 and is held to its own single-kernel bar against the restatement on those rounded values.  Chained: the same six
    launches back to back on device buffers are finite and give the same bits twice."""
    lib = _lib()
    sd, x, gvec, mask = R.chain_inputs()
    B, H, L, _ = R.CHAIN_SHAPE
    n = R.CHAIN_LAYERS
    ins, rss = R.chain_layers(sd)
    gl_all = R.cond(gvec, sd["wn.cond_layer.weight"], sd["wn.cond_layer.bias"]).float()
    steps = R.chain(x, gl_all, mask, ins, rss)
    for i, s in enumerate(steps):
        gl = gl_all[:, 2 * H * i:2 * H * (i + 1)]
        x32 = s["x_in"].float()
        v = R.preact(x32, ins[i][0], ins[i][1], gl)
        rc, acts = wn_in_layer(lib, x32, ins[i][0], ins[i][1], gl, 0)
        assert rc == 0
        check_gate(f"teacher-forced layer {i} in_layer", acts.cpu(), R.gate(v, H), v)
        o32 = None if i == 0 else s["out_in"].float()
        check_res_skip(f"teacher-forced layer {i} res_skip", lib, s["acts"].float(), rss[i][0], rss[i][1], x32, o32, mask, 0, i == 0,
                       i == n - 1)

    def run():
        xd, md = x.cuda(), mask.cuda()
        acts, od = nan(B * H + GUARD, L), nan(B, H, L)
        for i in range(n):
            rc, _ = wn_in_layer(lib, x, ins[i][0], ins[i][1], gl_all[:, 2 * H * i:2 * H * (i + 1)], 0, xd=xd, acts=acts)
            assert rc == 0
            assert wn_res_skip(lib, acts, rss[i][0], rss[i][1], xd, od, md, 0, i == 0, i == n - 1) == 0
        return od.cpu(), xd.cpu()
    o1, x1 = run()
    o2, x2 = run()
    err = R.rel_err(o1, steps[-1]["out"])
    print(f"\n[chained 3 layers] rel_err vs the fp64 chain {err:.3e} (reported, no bar: three layers of accumulated error)")
    assert torch.isfinite(o1).all() and torch.isfinite(x1).all()
    assert torch.equal(o1, o2) and torch.equal(x1, x2)


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_gate_refusals_launch_nothing():
    """ACT_GATE with a K split, a residual, a mask, cout % 32 != 0 or an x6 / x3 tile: -1, and the output is still all NaN.  bv2_test_conv1d
    checks none of this itself: it packs, uploads and hands the launch to launch_conv1d as asked, so the -1 is the launcher's, and a
    launcher that let one through would return 0 and write the output."""
    lib = _lib()
    B, H, L = 1, 64, 40
    x, w, b, gl = R.in_inputs(B, H, L)
    res, om = torch.zeros(B, H, L, device="cuda"), torch.ones(B, L, device="cuda")
    cases = {"ksplit 2": dict(tile=6, ksplit=2), "res add": dict(res=res, res_mode=1), "res rsub": dict(res=res, res_mode=2),
             "out_mask": dict(out_mask=om), "mask_pre": dict(out_mask=om, mask_pre=1), "mask_post": dict(out_mask=om, mask_post=1),
             "mask_pre alone": dict(mask_pre=1), "mask_post alone": dict(mask_post=1), "x6": dict(tile=8), "x6 128x64": dict(tile=9), "x3": dict(tile=14)}
    for name, kw in cases.items():
        rc, buf = gate_conv1d(lib, x, w, b, gl, kw.pop("tile", 0), **kw)
        print(f"\n[refusal {name}] status {rc}")
        assert rc == -1 and torch.isnan(buf).all(), name
    rc, buf = gate_conv1d(lib, x, w[:48], b[:48], gl[:, :48], 0)       # cout = 48: a ragged (tanh, sigmoid) tile
    print(f"\n[refusal cout 48] status {rc}")
    assert rc == -1 and torch.isnan(buf).all()
    rc, buf = gate_conv1d(lib, x, w, b, gl, 0)                          # ... and the same call without any of them runs
    assert rc == 0 and torch.isfinite(buf[:B * H]).all()
