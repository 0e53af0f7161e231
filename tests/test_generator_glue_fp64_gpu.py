"""GPU: the Generator's stage glue at kernel level against fp64 restatements (plain torch calls) — the launches between the ResBlock pairs
that so far were held only by end-to-end waveform bars and one tap at T_y ~ 20:

* ConvTranspose1d, fp32: the executor's own ConvLaunch of u polyphase problems (ups_conv_launch through bv2_test_conv_transpose) on the
  LDS-tiled kernel and on the split-K kernel, for all 22 (u, k) pairs of the envelope, the released stages, every column-tile edge and the
  per-XCD column permutation, with exact lengths, single phases and the shared max |out| slot;
* multi-problem ConvLaunches (bv2_test_conv_multi): problems of different k on the plain grid, the per-XCD ranges and the cost-sorted snake
  of conv_mfma.hip and conv_x6.hip, and the two-problem split-K launch of enc_p.proj;
* ConvTranspose1d, bf16 channels-last (ups_cl_launch through bv2_test_conv_transpose_cl), per-phase tap restriction on and off;
* conv_post + tanh, fp32 (kernels/misc.hip) and bf16 (kernels/gen_bf16.hip), both kernels of each.

Bars (none measured first): fp32 kernels max |got - ref| <= 2e-5 max |ref| (tests/test_kernels_gpu.py); x6 tiles additionally at most twice
the fp32-MFMA kernel's own error on the same launch + 2e-7 (tests/test_x6_gpu.py); bf16 outputs |err| <= 2^-8 |ref| + 2e-5 max |ref|
elementwise (test_conv_cl_bf16_kernel); conv_post max |got - ref| <= 2e-5 max(1, max |pre-tanh sum|) (tanh is 1-Lipschitz).  Everything else
(residue classes, guard bands, the max |out| slot, alone-vs-ragged, tap restriction on / off) is exact.

Every output buffer is NaN-filled with a guard band of sentinels on either side that must survive; only an item's valid columns
[0, lens[b] * len_mul * out_tstride) are compared (the LDS-tiled kernel skips tiles past an item's end, the split-K kernel does not)."""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

PAIRS = [(u, u * r) for u in range(2, 9) for r in range(1, 5) if (u * r - u) % 2 == 0]       # the envelope's 22 (u, k)
PLAIN, PER_XCD, SNAKE = 0, 1, 2                                                                # bv2_kernels.h PLACE_*
GUARD, SENTINEL = 256, 12288.0        # exact in bf16 too
BN = {1: 128, 2: 128, 3: 64, 4: 128, 5: 256, 7: 64}                                            # column tile of each LDS-tiled tile id


class Prob(C.Structure):                                                                      # bv2_testing.h bv2_test_conv_prob
    _fields_ = [("w_host", C.c_void_p), ("bias_host", C.c_void_p), ("k", C.c_int32), ("dil", C.c_int32), ("pad_left", C.c_int32),
                ("out", C.c_void_p), ("out_rstride", C.c_int32), ("out_tstride", C.c_int32), ("out_toff", C.c_int32),
                ("res", C.c_void_p), ("res_mode", C.c_int32)]


def _lib():
    from bert_vits2_amd import lib as L
    lib = L.load()
    i, p, f, i64 = C.c_int, C.c_void_p, C.c_float, C.c_int64
    lib.bv2_test_conv_multi_pack_floats.restype = i64
    lib.bv2_test_conv_multi_pack_floats.argtypes = [i, i, p, i]
    lib.bv2_test_conv_multi.restype = i
    lib.bv2_test_conv_multi.argtypes = [p, p, i, i, i, p, p, p, i, f, f, p, i, i, i, i, i, i64, p, p, p, p]
    lib.bv2_test_conv_transpose_pack_floats.restype = i64
    lib.bv2_test_conv_transpose_pack_floats.argtypes = [i] * 4
    lib.bv2_test_conv_transpose.restype = i
    lib.bv2_test_conv_transpose.argtypes = [p, p, p, i, i, i, i, p, p, p, i, p, p, i, i, i, i, i, p, p, p]
    lib.bv2_test_conv_transpose_cl_pack_bytes.restype = i64
    lib.bv2_test_conv_transpose_cl_pack_bytes.argtypes = [i] * 4
    lib.bv2_test_conv_transpose_cl.restype = i
    lib.bv2_test_conv_transpose_cl.argtypes = [p, p, p, i, i, i, i, p, p, p, i, p, p, i, i, i, i, p]
    lib.bv2_test_conv_post.restype = i
    lib.bv2_test_conv_post.argtypes = [p, p, p, p, i, p, p, p, p, i, i, i, i, i]
    lib.bv2_test_conv_post_cl.restype = i
    lib.bv2_test_conv_post_cl.argtypes = [p, p, p, p, i, p, p, p, p, i, i, i, i, i, i]
    return lib


def P(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def guarded(shape, dtype=torch.float32):
    """a NaN-filled device tensor inside a buffer with GUARD sentinels in front and behind"""
    n = math.prod(shape)
    buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=dtype, device="cuda")
    buf[GUARD:GUARD + n] = float("nan")
    return buf, buf[GUARD:GUARD + n].view(shape)


def guard_intact(buf):
    return bool((buf[:GUARD] == SENTINEL).all() and (buf[-GUARD:] == SENTINEL).all())


def valid_mask(lens, len_mul, L, B):
    """[B][L] bool: the input columns of each item that exist"""
    le = torch.full((B,), L, dtype=torch.int64) if lens is None else torch.tensor(lens, dtype=torch.int64) * len_mul
    return torch.arange(L)[None, :] < le.clamp(max=L)[:, None]


def lrelu64(x, slope):
    return torch.where(x < 0, x * slope, x)


def f32c(v):
    return torch.tensor(v, dtype=torch.float32)


def bfr(t):                                           # fp32 -> nearest bf16, kept in fp32
    return t.to(torch.bfloat16).to(torch.float32)


def stage_mean_bf16(xs):
    """cl_bf16.h stage_mean on fp32 tensors that hold bf16 values: the branch mean with the kernels' rounding points"""
    if len(xs) == 1:
        return xs[0]
    s = bfr(xs[2] + xs[1]) + xs[0] if len(xs) == 3 else xs[1] + xs[0]
    return bfr(s * (f32c(1.0) / f32c(float(len(xs)))))


def slot_value(slot):                                 # ConvProb::omax: one word per XCD, 32 words apart; the value is their max
    return slot[::32].contiguous().max().view(torch.float32).item()


# ------------------------------------------------------------------------------------------------------------------------------------------
# ConvTranspose1d, fp32
def ct_inputs(cin, cout, u, k, nsrc, B, L, seed):
    g = torch.Generator().manual_seed(seed)
    xs = [torch.randn(B, cin, L, generator=g) for _ in range(nsrc)]
    w = torch.randn(cin, cout, k, generator=g) / math.sqrt(cin * (k // u))
    b = torch.randn(cout, generator=g)
    return xs, w, b


def ct_ref(xs, w, b, u, k, lens, len_mul):
    B, _, L = xs[0].shape
    m = sum(x.double() for x in xs) / len(xs) * valid_mask(lens, len_mul, L, B)[:, None, :]
    return F.conv_transpose1d(lrelu64(m, 0.1), w.double(), b.double(), stride=u, padding=(k - u) // 2)


def ct_run(lib, xs, w, b, u, k, lens=None, len_mul=1, tile=0, only_phase=-1, slot=None):
    B, cin, L = xs[0].shape
    cout = w.shape[1]
    xd = [x.cuda() for x in xs] + [None, None]
    buf, out = guarded((B, cout, L * u))
    wp = torch.empty(lib.bv2_test_conv_transpose_pack_floats(u, k, cin, cout), device="cuda")
    ld = None if lens is None else torch.tensor(lens, dtype=torch.int64).cuda()
    info = torch.full((2,), -1, dtype=torch.int32)
    rc = lib.bv2_test_conv_transpose(None, P(w.contiguous()), P(b), u, k, cin, cout, P(xd[0]), P(xd[1]), P(xd[2]), len(xs), P(out), P(ld),
                                     len_mul, B, L, tile, only_phase, P(slot), P(wp), P(info))
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert guard_intact(buf)
    return out.cpu(), int(info[0])


def check_fp32(got, ref, vmask, tag, bar=2e-5):
    """max |got - ref| <= bar * max |ref| over the valid columns, all of which must have been written"""
    vm = vmask[:, None, :].expand_as(ref)
    assert torch.isfinite(got[vm]).all(), tag
    e = ((got.double() - ref)[vm].abs().max() / ref[vm].abs().max()).item()
    print(f"\n[{tag}] max |err| / max |ref| = {e:.2e}")
    assert e <= bar, (tag, e)
    return e


def ct_case(lib, cin, cout, u, k, nsrc, B, L, lens, len_mul, tile, tag):
    xs, w, b = ct_inputs(cin, cout, u, k, nsrc, B, L, 1000 * u + 10 * k + L + nsrc)
    got, place = ct_run(lib, xs, w, b, u, k, lens, len_mul, tile)
    vout = valid_mask(lens, len_mul, L, B).repeat_interleave(u, dim=1)
    check_fp32(got, ct_ref(xs, w, b, u, k, lens, len_mul), vout, tag)
    return place


@pytest.mark.parametrize("u,k", PAIRS)
def test_conv_transpose_every_envelope_pair(u, k):
    """nsrc = 3 on the product's pick (LDS-tiled) and nsrc = 1 on the split-K kernel (what stage 0 runs at batch 1), ragged"""
    lib = _lib()
    ct_case(lib, 32, 16, u, k, 3, 2, 37, [37, 9], 1, 0, f"ct fp32 lds u={u} k={k}")
    ct_case(lib, 32, 16, u, k, 1, 2, 37, [37, 9], 1, 6, f"ct fp32 splitk u={u} k={k}")


STAGES = [(512, 256, 8, 16, 1, 24), (512, 256, 8, 16, 1, 384), (256, 128, 8, 16, 3, 96), (128, 64, 2, 4, 3, 517), (64, 32, 2, 4, 3, 1030),
          (32, 16, 2, 4, 3, 2063)]


@pytest.mark.parametrize("cin,cout,u,k,nsrc,L", STAGES)
def test_conv_transpose_released_stages(cin, cout, u, k, nsrc, L):
    lib = _lib()
    ct_case(lib, cin, cout, u, k, nsrc, 1, L, None, 1, 0, f"ct fp32 stage {cin}->{cout} L={L} B=1")
    n = L // 8                                          # ragged, 8 samples per latent frame: item 0 ends at 8 n <= L, item 1 well inside
    ct_case(lib, cin, cout, u, k, nsrc, 2, L, [n, max(1, (2 * n) // 5)], 8, 0, f"ct fp32 stage {cin}->{cout} L={L} ragged")


@pytest.mark.parametrize("tile", sorted(BN))
def test_conv_transpose_column_tile_edges_and_per_xcd_ranges(tile):
    """one tile short / exact / one over, whole multiples of 8 tiles (per-XCD ranges), and ntx >= 64 with a ragged last tile and idle
    padding workgroups; the placement is the launcher's own report"""
    lib = _lib()
    bn = BN[tile]
    seen = set()
    for L in (1, bn - 1, bn, bn + 1, 8 * bn, 16 * bn, 65 * bn - 17):
        place = ct_case(lib, 64, 64, 2, 4, 3, 1, L, None, 1, tile, f"ct fp32 tile {tile} L={L}")
        ntx = (L + bn - 1) // bn
        assert place == (PER_XCD if ntx % 8 == 0 or ntx >= 64 else PLAIN), (tile, L, ntx, place)
        seen.add(place)
    assert seen == {PLAIN, PER_XCD}


@pytest.mark.parametrize("u,k,nsrc,tile", [(8, 16, 3, 0), (3, 9, 3, 0), (8, 16, 1, 6), (2, 4, 1, 6)])
def test_conv_transpose_single_phase_writes_its_residue_class_alone(u, k, nsrc, tile):
    lib = _lib()
    B, L, lens = 2, 37, [37, 9]
    xs, w, b = ct_inputs(32, 16, u, k, nsrc, B, L, 77 * u + k)
    full, _ = ct_run(lib, xs, w, b, u, k, lens, 1, tile)
    vout = valid_mask(lens, 1, L, B).repeat_interleave(u, dim=1)[:, None, :].expand_as(full)
    assert torch.isfinite(full[vout]).all()
    t = torch.arange(L * u)
    for ph in range(u):
        one, _ = ct_run(lib, xs, w, b, u, k, lens, 1, tile, only_phase=ph)
        assert torch.isnan(one[:, :, t % u != ph]).all(), ph
        mine = vout & (t % u == ph)[None, None, :]
        assert torch.equal(one[mine], full[mine]), ph


@pytest.mark.parametrize("u,k,nsrc,tile,L", [(8, 16, 3, 0, 37), (2, 4, 3, 3, 1100), (8, 16, 1, 6, 37), (4, 8, 1, 6, 200)])
def test_conv_transpose_phases_share_one_max_abs_slot(u, k, nsrc, tile, L):
    """the u problems publish into ONE ConvProb::omax slot: exactly the largest stored magnitude (lens = NULL)"""
    lib = _lib()
    xs, w, b = ct_inputs(32, 16, u, k, nsrc, 2, L, 5 * u + k + L)
    slot = torch.zeros(256, dtype=torch.int32, device="cuda")
    got, _ = ct_run(lib, xs, w, b, u, k, None, 1, tile, slot=slot)
    assert torch.isfinite(got).all()
    assert slot_value(slot) == got.abs().max().item()


@pytest.mark.parametrize("cin,cout,u,k,nsrc,tile,lens,len_mul", [
    (32, 16, 8, 16, 3, 4, [37, 9], 1), (64, 64, 2, 4, 3, 3, [13, 5], 8), (128, 64, 2, 4, 3, 2, [40, 17], 8), (32, 16, 3, 9, 3, 5, [70, 33], 4),
    (32, 16, 8, 16, 1, 6, [37, 9], 1), (512, 256, 8, 16, 1, 6, [3, 1], 8), (64, 32, 4, 8, 1, 6, [13, 5], 8)])
def test_conv_transpose_ragged_item_equals_the_item_alone(cin, cout, u, k, nsrc, tile, lens, len_mul):
    """bv2_kernels.h: with lens a batch item is computed "exactly as if the utterance had been run alone" — bit for bit, same tile"""
    lib = _lib()
    B, L = 2, lens[0] * len_mul
    xs, w, b = ct_inputs(cin, cout, u, k, nsrc, B, L, cin + 3 * u + k)
    both, _ = ct_run(lib, xs, w, b, u, k, lens, len_mul, tile)
    for i in range(B):
        Li = lens[i] * len_mul
        alone, _ = ct_run(lib, [x[i:i + 1, :, :Li].contiguous() for x in xs], w, b, u, k, None, 1, tile)
        assert torch.isfinite(alone).all()
        assert torch.equal(both[i, :, :Li * u], alone[0]), i


# ------------------------------------------------------------------------------------------------------------------------------------------
# multi-problem ConvLaunches
def multi_run(lib, x, ws, bs, ks, dils, tile, lens=None, slope=0.1, res=True, ksplit=1, out_mask=None):
    """problems i = conv(lrelu(x), ws[i], dil[i]) + bs[i] (+ x); returns the outputs in the order given [ksplit slabs summed], placement, ksplit"""
    B, cin, L = x.shape
    cout = ws[0].shape[0]
    xd = x.cuda()
    n = len(ws)
    kt = torch.tensor(ks, dtype=torch.int32)
    wp = torch.empty(lib.bv2_test_conv_multi_pack_floats(cin, cout, P(kt), n), device="cuda")
    slabs = 8 if ksplit != 1 else 1
    outs = [guarded((slabs, B, cout, L)) for _ in range(n)]
    keep = [w.contiguous() for w in ws]
    probs = (Prob * n)()
    for i in range(n):
        probs[i] = Prob(keep[i].data_ptr(), bs[i].data_ptr(), ks[i], dils[i], -1, outs[i][1].data_ptr(), L, 1, 0,
                        xd.data_ptr() if res else None, 1 if res else 0)
    ld = None if lens is None else torch.tensor(lens, dtype=torch.int64).cuda()
    md = None if out_mask is None else out_mask.float().cuda()
    info = torch.full((2,), -1, dtype=torch.int32)
    rc = lib.bv2_test_conv_multi(None, probs, n, cin, cout, P(xd), None, None, 1, 1.0, slope, P(ld), 1, B, L, tile, ksplit, B * cout * L, P(md),
                                 None, P(wp), P(info))
    assert rc == 0, rc
    torch.cuda.synchronize()
    place, ks_used = int(info[0]), int(info[1])
    assert all(guard_intact(buf) for buf, _ in outs)
    got = []
    for _, o in outs:
        o = o.cpu()
        assert torch.isnan(o[ks_used:]).all()                                  # slabs the launch was not asked for stay untouched
        got.append(o[:ks_used].sum(0) if ks_used > 1 else o[0])
    return got, place, ks_used


def branch_inputs(C_, B, L, ks, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, C_, L, generator=g)
    ws = {k: torch.randn(C_, C_, k, generator=g) / math.sqrt(C_ * k) for k in ks}
    bs = {k: torch.randn(C_, generator=g) for k in ks}
    return x, ws, bs


def branch_refs(x, ws, bs, dil, lens):
    B, _, L = x.shape
    xin = lrelu64(x.double() * valid_mask(lens, 1, L, B)[:, None, :], 0.1)
    return {k: F.conv1d(xin, ws[k].double(), bs[k].double(), padding=(k - 1) // 2 * dil[k], dilation=dil[k]) + x.double() for k in ws}


DIL = {3: 1, 7: 3, 11: 5}
BRANCH_SHAPES_C64 = [(1, 700, None, PLAIN), (1, 5632, None, SNAKE), (1, 5807, None, SNAKE), (2, 3072, [3072, 1100], SNAKE)]


@pytest.mark.parametrize("B,L,lens,place", BRANCH_SHAPES_C64)
def test_resblock_branch_set_on_conv_mfma_in_either_order(B, L, lens, place):
    """k = 3 / 7 / 11 with dilations 1 / 3 / 5, pre-lrelu, residual, C = 64, the 64 x 64 tile: off the snake (11 column tiles) and on it (88
    tiles = 264 workgroups; 91 tiles = padding workgroups; a ragged batch) — each output must be ITS problem's, however the launch sorts"""
    lib = _lib()
    x, ws, bs = branch_inputs(64, B, L, (3, 7, 11), L + B)
    refs = branch_refs(x, ws, bs, DIL, lens)
    vm = valid_mask(lens, 1, L, B)
    res = {}
    for order in ((3, 7, 11), (11, 7, 3)):
        got, p, _ = multi_run(lib, x, [ws[k] for k in order], [bs[k] for k in order], list(order), [DIL[k] for k in order], 3, lens)
        assert p == place, (p, place)
        for k, o in zip(order, got):
            check_fp32(o, refs[k], vm, f"multi fp32 C=64 L={L} B={B} order={order} k={k}")
        res[order] = dict(zip(order, got))
    vx = vm[:, None, :].expand(B, 64, L)
    for k in (3, 7, 11):
        assert torch.equal(res[(3, 7, 11)][k][vx], res[(11, 7, 3)][k][vx]), k


@pytest.mark.parametrize("tile,B,L,lens", [(9, 1, 5632, None), (9, 1, 5807, None), (9, 2, 3072, [3072, 1100]),
                                           # the 64 x 128 tile: 2 row tiles, 128 columns — 48 / 65 column tiles at B = 1 give 288 / 432 workgroups
                                           (11, 1, 6144, None), (11, 1, 8303, None), (11, 2, 3072, [3072, 1100]),
                                           # the two-plane fp16 form ("x3") of the 128 x 64 tile, max |x| slots filled by the entry point
                                           (14, 1, 5632, None), (14, 1, 5807, None), (14, 2, 3072, [3072, 1100])])
def test_resblock_branch_set_on_conv_x6_snake(tile, B, L, lens):
    """the same three-branch launch at C = 128 on the bf16 matrix core (conv_x6.hip places like conv_mfma.hip, snake for 256 < workgroups <=
    512): test_x6_gpu.py's one-problem bars against the fp32-MFMA kernel's own error on the same launch"""
    lib = _lib()
    x, ws, bs = branch_inputs(128, B, L, (3, 7, 11), L + B + tile)
    refs = branch_refs(x, ws, bs, DIL, lens)
    vm = valid_mask(lens, 1, L, B)
    res = {}
    for order in ((3, 7, 11), (11, 7, 3)):
        args = ([ws[k] for k in order], [bs[k] for k in order], list(order), [DIL[k] for k in order])
        got, p, _ = multi_run(lib, x, *args, tile, lens)
        assert p == SNAKE, p
        g32, _, _ = multi_run(lib, x, *args, 3, lens)
        for k, o, o32 in zip(order, got, g32):
            tag = f"multi x6 tile={tile} L={L} B={B} order={order} k={k}"
            e6 = check_fp32(o, refs[k], vm, tag)
            e32 = check_fp32(o32, refs[k], vm, tag + " (fp32-MFMA)")
            assert e6 <= 2.0 * e32 + 2e-7, (tag, e6, e32)
        res[order] = dict(zip(order, got))
    vx = vm[:, None, :].expand(B, 128, L)
    for k in (3, 7, 11):
        assert torch.equal(res[(3, 7, 11)][k][vx], res[(11, 7, 3)][k][vx]), k


@pytest.mark.parametrize("L", [24, 77])
@pytest.mark.parametrize("ksplit", [1, 0, 2])          # none, the executor's pick (conv_pick_ksplit), two partial slabs
def test_two_problem_splitk_launch_like_enc_p_proj(L, ksplit):
    """run_encode's m_p / logs_p halves: two 1 x 1 problems 192 -> 192 on one input, masked output, one split-K launch"""
    lib = _lib()
    g = torch.Generator().manual_seed(L)
    B, C_ = 2, 192
    x = torch.randn(B, C_, L, generator=g)
    ws = [torch.randn(C_, C_, 1, generator=g) / math.sqrt(C_) for _ in range(2)]
    bs = [torch.randn(C_, generator=g) for _ in range(2)]
    mask = valid_mask([L, L // 3], 1, L, B)
    got, place, ks = multi_run(lib, x, ws, bs, [1, 1], [1, 1], 6, None, slope=0.0, res=False, ksplit=ksplit, out_mask=mask)
    assert place == PER_XCD and (ks == ksplit or ksplit == 0) and 1 <= ks <= 8
    full = torch.ones(B, L, dtype=torch.bool)
    for i in range(2):
        ref = F.conv1d(x.double(), ws[i].double(), bs[i].double()) * mask[:, None, :]
        check_fp32(got[i], ref, full, f"multi splitk enc_p.proj L={L} ksplit={ks} problem {i}")
        assert (got[i][~mask[:, None, :].expand_as(ref)] == 0).all()


# ------------------------------------------------------------------------------------------------------------------------------------------
# ConvTranspose1d, bf16 channels-last
def ctcl_run(lib, xs, w, b, u, k, lens, len_mul, phase_taps):
    B, cin, L = xs[0].shape
    cout = w.shape[1]
    xd = [x.transpose(1, 2).contiguous().to(torch.bfloat16).cuda() for x in xs] + [None, None]
    buf, out = guarded((B, L * u, cout), torch.bfloat16)
    wp = torch.zeros(lib.bv2_test_conv_transpose_cl_pack_bytes(u, k, cin, cout) + 8192, dtype=torch.uint8, device="cuda")
    ld = None if lens is None else torch.tensor(lens, dtype=torch.int64).cuda()
    rc = lib.bv2_test_conv_transpose_cl(None, P(w.contiguous()), P(b), u, k, cin, cout, P(xd[0]), P(xd[1]), P(xd[2]), len(xs), P(out), P(ld),
                                        len_mul, B, L, phase_taps, P(wp))
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert guard_intact(buf)
    return out.float().cpu().transpose(1, 2)


def ctcl_case(lib, cin, cout, u, k, nsrc, B, L, lens, len_mul):
    g = torch.Generator().manual_seed(900 * u + 7 * k + L)
    xs = [bfr(torch.randn(B, cin, L, generator=g)) for _ in range(nsrc)]
    w = torch.randn(cin, cout, k, generator=g) / math.sqrt(cin * (k // u))
    b = torch.randn(cout, generator=g)
    m = stage_mean_bf16(xs)
    pre = bfr(torch.where(m < 0, m * f32c(0.1), m)).double() * valid_mask(lens, len_mul, L, B)[:, None, :]
    ref = F.conv_transpose1d(pre, bfr(w).double(), b.double(), stride=u, padding=(k - u) // 2)
    vm = valid_mask(lens, len_mul, L, B).repeat_interleave(u, dim=1)[:, None, :].expand_as(ref)
    scale = ref[vm].abs().max().item()
    got = {}
    for taps in (1, 0):
        o = ctcl_run(lib, xs, w, b, u, k, lens, len_mul, taps)
        assert torch.isfinite(o[vm]).all()
        err = (o.double() - ref)[vm].abs()
        worst = (err / (2.0 ** -8 * ref[vm].abs() + 2e-5 * scale)).max().item()
        print(f"\n[ct bf16 {cin}->{cout} u={u} k={k} L={L} B={B} phase_taps={taps}] max |err| / (2^-8 |ref| + 2e-5 max |ref|) = {worst:.3f}")
        assert worst <= 1.0, (taps, worst)
        got[taps] = o
    assert torch.equal(got[1][vm], got[0][vm])         # stepping over the window's zero taps changes nothing, bit for bit


@pytest.mark.parametrize("u,k", PAIRS)
def test_conv_transpose_cl_bf16_every_envelope_pair(u, k):
    ctcl_case(_lib(), 32, 16, u, k, 3, 1, 131, None, 1)


@pytest.mark.parametrize("cin,cout,u,k,nsrc,B,L,lens,len_mul", [(512, 256, 8, 16, 1, 1, 40, None, 1), (32, 16, 2, 4, 3, 2, 515, [64, 25], 8)])
def test_conv_transpose_cl_bf16_released_stages(cin, cout, u, k, nsrc, B, L, lens, len_mul):
    ctcl_case(_lib(), cin, cout, u, k, nsrc, B, L, lens, len_mul)


# ------------------------------------------------------------------------------------------------------------------------------------------
# conv_post + tanh
def post_weight(C_, k, nsrc, g):
    """w [C][k] scaled so that the pre-tanh sum has unit spread on this input distribution: tanh's linear and saturated regions both occur"""
    w = torch.randn(C_, k, generator=g)
    xs = [torch.randn(1, C_, 4000, generator=g) for _ in range(nsrc)]
    a = F.conv1d(lrelu64(sum(x.double() for x in xs) / nsrc, 0.01), w.double()[None], padding=(k - 1) // 2)
    return (w / a.std().item()).contiguous()


def post_ref(xs, w, lens, len_mul, bf16):
    B, _, L = xs[0].shape
    if bf16:
        m = stage_mean_bf16(xs)
        pre = torch.where(m < 0, m * f32c(0.01), m).double()
    else:
        pre = lrelu64(sum(x.double() for x in xs) / len(xs), 0.01)
    a = F.conv1d(pre * valid_mask(lens, len_mul, L, B)[:, None, :], w.double()[None], padding=(w.shape[1] - 1) // 2)[:, 0]
    return torch.tanh(a), a


def post_run(lib, xs, w, lens, len_mul, bf16, generic=0):
    B, C_, L = xs[0].shape
    k = w.shape[1]
    if bf16:
        xd = [x.transpose(1, 2).contiguous().to(torch.bfloat16).cuda() for x in xs] + [None, None]
    else:
        xd = [x.cuda() for x in xs] + [None, None]
    buf, out = guarded((B, L))
    wd = torch.empty(C_ * k, device="cuda")
    ld = None if lens is None else torch.tensor(lens, dtype=torch.int64).cuda()
    if bf16:
        rc = lib.bv2_test_conv_post_cl(None, P(xd[0]), P(xd[1]), P(xd[2]), len(xs), P(w), P(wd), P(out), P(ld), len_mul, B, C_, k, L, generic)
    else:
        rc = lib.bv2_test_conv_post(None, P(xd[0]), P(xd[1]), P(xd[2]), len(xs), P(w), P(wd), P(out), P(ld), len_mul, B, C_, k, L)
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert guard_intact(buf)
    return out.cpu()


def post_cases(edge):
    """(B, L, lens, len_mul): lengths around one workgroup's `edge` outputs, and ragged items whose valid end falls on the edge and inside a halo"""
    for L in (1, edge - 1, edge, edge + 1, 1000):
        yield 1, L, None, 1
    for end in (edge, edge - 3, edge + 3):
        yield 2, 2 * edge + 40, [2 * edge + 40, end], 1
    yield 2, 600, [300, edge // 2], 2


def post_check(lib, C_, nsrc, bf16, generic, edges, tag):
    g = torch.Generator().manual_seed(31 * C_ + nsrc + 2 * generic)
    w = post_weight(C_, 7, nsrc, g)
    worst = 0.0
    for edge in edges:
        for B, L, lens, len_mul in post_cases(edge):
            xs = [torch.randn(B, C_, L, generator=g) for _ in range(nsrc)]
            xs = [bfr(x) for x in xs] if bf16 else xs
            ref, a = post_ref(xs, w, lens, len_mul, bf16)
            got = post_run(lib, xs, w, lens, len_mul, bf16, generic)
            vm = valid_mask(lens, len_mul, L, B)
            assert torch.isfinite(got[vm]).all(), (L, lens)
            e = (got.double() - ref)[vm].abs().max().item() / max(1.0, a[vm].abs().max().item())
            assert e <= 2e-5, (tag, B, L, lens, len_mul, e)
            worst = max(worst, e)
            if L >= 1000:                                # both regions of tanh are in play
                assert (ref.abs() < 0.3).any() and (ref.abs() > 0.9).any()
    print(f"\n[{tag}] max |err| / max(1, max |pre-tanh|) = {worst:.2e}")


@pytest.mark.parametrize("nsrc", [1, 2, 3])
@pytest.mark.parametrize("C_", [16, 32, 64])             # 16: conv_post_c_kernel<16>; 32 / 64: conv_post_kernel (the envelope's other final widths)
def test_conv_post_fp32(C_, nsrc):
    post_check(_lib(), C_, nsrc, False, 0, (256,), f"conv_post fp32 C={C_} nsrc={nsrc}")


@pytest.mark.parametrize("nsrc", [1, 2, 3])
@pytest.mark.parametrize("C_,generic", [(16, 0), (16, 1), (32, 0), (64, 0)])
def test_conv_post_cl_bf16(C_, generic, nsrc):
    """C = 16 row-wise (conv_post_cl16_kernel<7>: 250 outputs per workgroup) and the any-width kernel (256), ragged ends around both"""
    rows = C_ == 16 and not generic
    post_check(_lib(), C_, nsrc, True, generic, (250, 256), f"conv_post bf16 C={C_} {'rows' if rows else 'any-width'} nsrc={nsrc}")
