"""CPU: the packer's host number formats (csrc/bv2_kernels.h f2bf / f2h / h2f, one definition each, through
include/bv2_testing.h bv2_test_convert) against torch's CPU conversions, bit for bit."""
import torch

from bert_vits2_amd import lib as L

F2BF, F2H, H2F = 0, 1, 2


def _convert(kind, src, out_dtype):
    lib = L.load()
    src = src.contiguous()
    out = torch.empty(src.numel(), dtype=out_dtype)
    assert lib.bv2_test_convert(kind, src.data_ptr(), out.data_ptr(), src.numel()) == 0
    return out


def _f32(bits):
    return torch.tensor(bits, dtype=torch.int64).to(torch.int32).view(torch.float32)


def _inputs():
    g = torch.Generator().manual_seed(20240607)
    rnd = torch.randint(-2 ** 31, 2 ** 31, (100000,), generator=g, dtype=torch.int64).to(torch.int32).view(torch.float32)
    # exact halfway cases around 1.0 of both formats (bf16: 8 significand bits, spacing 2^-7 above 1 and 2^-8 below; fp16: 11 bits,
    # 2^-10 / 2^-11), each with its two fp32 neighbours — ties go to the even neighbour, everything else to the nearest
    ties = []
    for step in (2.0 ** -7, 2.0 ** -10):
        for m in range(8):
            ties += [1.0 + (2 * m + 1) * step / 2, 1.0 - (2 * m + 1) * step / 4]
    ties = torch.tensor(ties, dtype=torch.float64).to(torch.float32)
    assert bool((ties.double() != 1.0).all())
    ties = torch.cat([ties, torch.nextafter(ties, torch.tensor(2.0)), torch.nextafter(ties, torch.tensor(0.0))])
    ties = torch.cat([ties, -ties])
    special = torch.tensor([0.0, -0.0, float("inf"), -float("inf"), float("nan"), 3.4028234663852886e38, -3.4028234663852886e38,
                            # round up to inf: in fp16 from 65520 (the tie above the largest fp16, 65504) on ...
                            65519.996, 65520.0, 65520.004, 65536.0, 1e5, -65520.0,
                            # ... and just below it the largest fp16 survives
                            65504.0, 65519.0], dtype=torch.float32)
    # ... in bf16 from 0x7f7f8000 (the tie above the largest bf16) on; NaNs with the payload in the low half only
    bits = _f32([0x7f7f7fff, 0x7f7f8000, 0x7f7f8001, 0x7f7fffff, 0xff7f8000, 0x7f800001, 0xff800001, 0x7fc00000, 0x7fffffff])
    return torch.cat([rnd, ties, special, bits])


def _check_h2f_every_fp16_pattern():
    bits = torch.arange(65536, dtype=torch.int32).to(torch.int16)
    ref = bits.view(torch.float16).to(torch.float32)
    got = _convert(H2F, bits, torch.float32)
    nan = torch.isnan(ref)
    assert int(nan.sum()) == 2 * 1023
    assert torch.equal(torch.isnan(got), nan), "NaN in, NaN out (and only then)"
    gb, rb = got.view(torch.int32), ref.view(torch.int32)
    assert torch.equal(gb[~nan], rb[~nan])
    quiet = 0x00400000                                # a signalling NaN may come back quiet; sign and the rest of the payload stay
    assert torch.equal(gb[nan] | quiet, rb[nan] | quiet)


def _check_narrowing(kind, dtype):
    x = _inputs()
    ref = x.to(dtype)
    got = _convert(kind, x, torch.int16).view(dtype)
    nan = torch.isnan(x)
    assert int(nan.sum()) > 300                       # the random patterns alone hold ~390 NaNs
    assert torch.equal(torch.isnan(ref), nan)
    assert torch.equal(torch.isnan(got), nan), "NaN in, NaN out (and only then)"
    g, r = got.view(torch.int16)[~nan], ref.view(torch.int16)[~nan]
    bad = (g != r).nonzero().flatten()
    assert bad.numel() == 0, [(hex(int(x[~nan].view(torch.int32)[i]) & 0xffffffff), hex(int(g[i]) & 0xffff), hex(int(r[i]) & 0xffff))
                              for i in bad[:8]]
    assert int(torch.isinf(got).sum()) > int(torch.isinf(x).sum())       # the inputs DO hold finite values that round up to inf


def test_host_formats_match_torch():
    _check_h2f_every_fp16_pattern()
    _check_narrowing(F2BF, torch.bfloat16)
    _check_narrowing(F2H, torch.float16)
    lib = L.load()
    x = torch.zeros(4)
    assert lib.bv2_test_convert(3, x.data_ptr(), x.data_ptr(), 4) == -1          # no such kind
    assert lib.bv2_test_convert(F2BF, None, x.data_ptr(), 4) == -1
