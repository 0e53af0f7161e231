"""GPU: true peak (bv2_true_peak, kernels/truepeak.hip; ``audio.true_peak``, ``normalize_loudness(peak="true")``,
``serving.synthesize(peak="true")``).

The yardstick of the kernel is the merged resampler: ``true_peak(x)`` is ``max(|x|.max(), |audio.resample(x, r, F r)|.max())`` as fp32
BITS — lengths around the interpolator's reach (K = 36, 73 taps) and around the kernel's tile, both input formats, a ragged batch with NaN
padding under a batch stride larger than S, alone and at row 2.  Against the fp64 oracle (tests/r128_oracle.py) the bar comes from the
table: (2K + 2) 2^-24 max_p sum_j |T[p][j]| max|x| covers the fmaf chain and the fp32 rounding of the taps.  Faded sines read their
amplitude inside EBU Tech 3341's window, +0.2 / -0.4 dB."""
import functools
import math

import numpy as np
import pytest
import torch

from bert_vits2_amd import audio, lib as L, serving
from tests import r128_oracle as R
from tests.test_resample_gpu import KW, _utts, narrow_model

pytestmark = pytest.mark.gpu

TILE = L.TRUE_PEAK_TILE
LENGTHS = (1, 5, 36, 37, 73, TILE - 1, TILE, TILE + 1, 3 * TILE + 17)
RATES = (8000, 44100, 48000, 96000)


@functools.lru_cache(maxsize=None)
def signal(n, dtype, seed=0):
    """White noise up to 0.9: between the samples of a long item the interpolated signal rises above every sample."""
    rng = np.random.RandomState(1000 * seed + n)
    x = rng.uniform(-0.9, 0.9, n)
    if dtype == "int16":
        return torch.from_numpy(np.round(x * 32767).astype(np.int16))
    return torch.from_numpy(x.astype(np.float32))


def as_f32(x):
    return x.to(torch.float32) / 32768.0 if x.dtype == torch.int16 else x


def composed(x, lens, rate):
    """The parent commit's path: the whole oversampled signal written by the resampler, then max |.| over it and over the samples."""
    F = R.factor(rate)
    w = x if x.dim() == 2 else x[None]
    lens = [w.shape[1]] * w.shape[0] if lens is None else lens
    sample = torch.stack([as_f32(w[b, :n]).abs().amax() for b, n in enumerate(lens)])
    if F == 1:
        return sample
    y, yl = audio.resample(w, lens, rate, F * rate)
    assert yl.tolist() == [F * n for n in lens]
    return torch.maximum(sample, torch.stack([y[b, :F * n].abs().amax() for b, n in enumerate(lens)]))


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


# ---- 1. bit for bit against the resampler ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float32", "int16"])
@pytest.mark.parametrize("rate", RATES)
def test_true_peak_is_the_resamplers_peak_bit_for_bit(rate, dtype):
    above = 0
    for n in LENGTHS:
        x = signal(n, dtype).cuda()
        got, want = audio.true_peak(x, None, rate), composed(x, None, rate)
        assert got.shape == (1,) and got.dtype == torch.float32 and torch.equal(bits(got), bits(want)), (rate, dtype, n, got, want)
        above += int(float(got) > float(as_f32(x).abs().max()))
    assert above >= 3                                         # the interpolated peak, not the sample peak, decides the long items


@pytest.mark.parametrize("dtype", ["float32", "int16"])
def test_at_192k_true_peak_is_the_sample_peak(dtype):
    assert audio.true_peak_plan(192000) == (1, 0)
    for n in (1, TILE + 1, 3 * TILE + 17):
        x = signal(n, dtype).cuda()
        assert torch.equal(bits(audio.true_peak(x, None, 192000)), bits(as_f32(x).abs().amax()[None]))


@pytest.mark.parametrize("rate", [44100, 96000])
def test_ragged_batch_nan_padding_wide_stride_and_rows(rate):
    lens = [TILE + 1, 37, 3 * TILE + 17]
    xs = [signal(n, "float32", seed=1 + i) for i, n in enumerate(lens)]
    S = max(lens)
    wide = torch.full((3, S + 37), float("nan")).cuda()
    for b, x in enumerate(xs):
        wide[b, 5:5 + len(x)] = x.cuda()
    view = wide[:, 5:5 + S]                                   # batch stride S + 37, rows not 16-byte aligned, NaN behind every item
    got = audio.true_peak(view, torch.tensor(lens).cuda(), rate)
    assert not torch.isnan(got).any()
    want = composed(view, lens, rate)
    assert torch.equal(bits(got), bits(want)), (got, want)
    host = audio.true_peak(view.cpu(), lens, rate)            # host tensors, host lengths
    assert torch.equal(bits(host), bits(got))
    for b, x in enumerate(xs):                                # the same item alone: the same bits (item 2 sits at row 2)
        assert torch.equal(bits(audio.true_peak(x.cuda(), None, rate)), bits(got[b:b + 1])), b
    info = audio.loudness(view, lens, rate, true_peak=True)
    assert torch.equal(bits(info["true_peak"]), bits(got)) and (info["true_peak"] >= info["peak"]).all()


def test_an_item_of_length_zero_reads_zero_and_nan_samples_do_not_count():
    x = signal(TILE + 1, "float32").cuda()[None].repeat(2, 1)
    got = audio.true_peak(x, torch.tensor([0, 5]).cuda(), 48000)
    assert float(got[0]) == 0.0 and torch.equal(bits(got[1:]), bits(composed(x[1, :5], None, 48000)))
    # a NaN INSIDE an item is skipped by the maximum, as the sample peak of the meter skips it: what is left are the outputs it
    # does not reach
    y = signal(400, "float32").clone()
    y[200] = float("nan")
    got = audio.true_peak(y.cuda(), None, 48000)
    ov, _ = audio.resample(y.cuda(), None, 48000, 192000)
    want = torch.maximum(torch.nan_to_num(ov, nan=0.0).abs().amax(), torch.nan_to_num(y, nan=0.0).abs().amax().cuda())
    assert torch.equal(bits(got), bits(want[None]))
    assert float(audio.loudness(y.cuda(), None, 48000)["peak"]) == float(torch.nan_to_num(y, nan=0.0).abs().amax())
    z = signal(400, "float32").clone()
    z[7] = float("inf")
    assert float(audio.true_peak(z.cuda(), None, 48000)) == math.inf


# ---- 2. against the fp64 oracle ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float32", "int16"])
@pytest.mark.parametrize("rate", RATES)
def test_true_peak_against_the_fp64_oracle(rate, dtype):
    F = R.factor(rate)
    t64, t32 = audio.resample_taps(rate, F * rate, np.float64), audio.resample_taps(rate, F * rate)
    worst = 0.0
    for n in LENGTHS:
        x = signal(n, dtype)
        got = float(audio.true_peak(x.cuda(), None, rate))
        want, bound = R.true_peak(x.numpy(), t64), R.true_peak_bound(x.numpy(), t32)
        worst = max(worst, abs(got - want) / bound)
        assert abs(got - want) <= bound, (rate, dtype, n, got, want, bound)
    print(f"{rate} Hz {dtype}: worst |device - oracle| = {worst:.3f} of the bound (2K + 2) 2^-24 max_p sum|T| max|x|")


@pytest.mark.parametrize("k", range(len(R.SINES)))
def test_faded_sines_read_their_amplitude(k):
    amp, f, phase = R.SINES[k]
    x = R.faded_sine(amp, f, phase).astype(np.float32)
    got = float(audio.true_peak(torch.from_numpy(x), None, 48000))
    over = 20 * math.log10(got / amp)
    print(f"A = {amp}, fs * {f:.4f}, {phase} deg: {over:+.5f} dB of the amplitude (sample peak {20 * math.log10(np.abs(x).max() / amp):+.4f} dB)")
    assert R.EBU_TP_WINDOW[0] <= over <= R.EBU_TP_WINDOW[1]


# ---- 3. a true-peak ceiling ------------------------------------------------------------------------------------------------------------
def test_a_true_peak_ceiling_limits_the_gain():
    rate, ceiling_db = 48000, -1.0
    x = torch.from_numpy(R.faded_sine(0.9, 1 / 4, 45.0).astype(np.float32)).cuda()
    sp, tp = float(x.abs().max()), float(audio.true_peak(x, None, rate))
    assert abs(sp - 0.9 * math.sqrt(0.5)) <= 1e-3 and abs(tp - 0.9) <= 1e-3          # 0.636 on the samples, 0.9 between them
    ceiling = 10.0 ** (ceiling_db / 20.0)
    out, info = audio.normalize_loudness(x, None, rate, target_lufs=0.0, peak_ceiling_db=ceiling_db, peak="true")
    assert bool(info["limited"][0]) and not bool(info["silent"][0])
    assert float(info["true_peak"][0]) == tp and float(info["peak"][0]) == sp
    gain, want = float(info["gain"][0]), ceiling / tp
    print(f"true-peak ceiling: gain {gain!r}, ceiling / true peak {want!r}, relative difference {abs(gain - want) / want:.3e}")
    assert abs(gain - want) <= 2.0 ** -23 * want                                        # the fp32 rounding of an fp64 quotient
    assert torch.equal(out[0], x * info["gain"][0])
    after = float(audio.true_peak(out, None, rate))
    print(f"true peak of the output {after!r}, ceiling {ceiling!r}, ratio - 1 = {after / ceiling - 1:.3e}")
    assert after <= ceiling * (1 + 2.0 ** -22)
    # peak="sample" is today's call: the gain of the gate fed the SAMPLE peak, exactly (a target 6 LU up, where that ceiling is met too)
    out_s, info_s = audio.normalize_loudness(x, None, rate, target_lufs=6.0, peak_ceiling_db=ceiling_db, peak="sample")
    out_d, info_d = audio.normalize_loudness(x, None, rate, target_lufs=6.0, peak_ceiling_db=ceiling_db)
    m0 = audio.loudness_measure(x[None], None, rate, gate=False)
    lens = torch.tensor([x.numel()]).cuda()
    g = audio.loudness_gate(m0["block_ms"], lens, x.numel(), m0["peak"], rate, None, 1, 6.0, ceiling_db)
    assert torch.equal(bits(info_s["gain"]), bits(g["gain"])) and torch.equal(bits(info_d["gain"]), bits(g["gain"]))
    assert torch.equal(out_s, out_d) and "true_peak" not in info_s and bool(info_s["limited"][0])
    assert float(info_s["gain"][0]) > gain and float(audio.true_peak(out_s, None, rate)) > ceiling      # what the sample ceiling lets through
    # the gate fed the true peak is what peak="true" ran
    gt = audio.loudness_gate(m0["block_ms"], lens, x.numel(), info["true_peak"], rate, None, 1, 0.0, ceiling_db)
    assert torch.equal(bits(gt["gain"]), bits(info["gain"]))


# ---- 4. serving ----------------------------------------------------------------------------------------------------------------------------
SERVE = dict(max_batch=4, max_pad_ratio=1.5, **KW)


def _seeded(lengths=(17, 24)):
    out = _utts(list(lengths))
    for i, u in enumerate(out):
        u.seed = 2000 + i
    return out


@pytest.mark.parametrize("groups", [None, ["doc", "doc"]])
def test_synthesize_under_a_true_peak_ceiling(groups):
    m = narrow_model()
    rate = m.hp.sampling_rate
    plain = serving.synthesize(m, _seeded(), **SERVE)
    ceiling = 10.0 ** (-1.0 / 20.0)
    got, levels = serving.synthesize(m, _seeded(), target_lufs=-16.0, peak="true", return_levels=True, loudness_groups=groups, **SERVE)
    for i, (a, b, lv) in enumerate(zip(plain, got, levels)):
        tp = audio.true_peak(torch.from_numpy(a), None, rate)
        assert lv["true_peak"] == float(tp) and lv["peak"] == float(np.abs(a).max()) and lv["true_peak"] >= lv["peak"]
        assert np.array_equal(b, a * np.float32(lv["gain"]))
        print(f"utterance {i}: true peak {lv['true_peak']:.6f}, sample peak {lv['peak']:.6f}, gain {lv['gain']:.6f}, limited {lv['limited']}")
        assert lv["true_peak"] * lv["gain"] <= ceiling * (1 + 2.0 ** -22)
    if groups is not None:
        assert len({lv["gain"] for lv in levels}) == 1
    # peak="sample" is the call without the argument, to the bit
    one = serving.synthesize(m, _seeded(), target_lufs=-16.0, peak="sample", return_levels=True, loudness_groups=groups, **SERVE)
    two = serving.synthesize(m, _seeded(), target_lufs=-16.0, return_levels=True, loudness_groups=groups, **SERVE)
    assert all(np.array_equal(a, b) for a, b in zip(one[0], two[0])) and one[1] == two[1] and "true_peak" not in one[1][0]


def test_a_low_true_peak_ceiling_is_kept_and_bad_arguments_raise():
    m = narrow_model()
    got, levels = serving.synthesize(m, _seeded(), target_lufs=20.0, peak_ceiling_db=-6.0, peak="true", return_levels=True, **SERVE)
    ceiling = 10.0 ** (-6.0 / 20.0)
    for lv in levels:                                         # a target out of reach: every utterance sits at the ceiling, in dBTP
        assert lv["limited"] and abs(lv["gain"] - ceiling / lv["true_peak"]) <= 2.0 ** -23 * lv["gain"]
    with pytest.raises(ValueError, match="target_lufs"):
        serving.synthesize(m, _seeded(), peak="true", **SERVE)
    with pytest.raises(ValueError, match="peak must be one of"):
        serving.synthesize(m, _seeded(), target_lufs=-16.0, peak="rms", **SERVE)


def test_documents_under_a_true_peak_ceiling():
    """``synthesize_documents(peak="true")`` is ``synthesize(loudness_groups=documents, peak="true")`` joined with its pauses, bit for bit
    (the pattern of tests/test_assemble_gpu.py's document test), under a ceiling that binds; every document sits at it, in dBTP."""
    from tests import assemble_oracle as AO
    from tests.test_assemble_gpu import DOC_OF, IDENT, SERVE as DOC_SERVE, _documents, _seeded as _doc_utts, _shape
    m = narrow_model()
    kw = dict(target_lufs=20.0, peak_ceiling_db=-6.0, peak="true", as_pcm16=False)
    want, levels = serving.synthesize(m, _doc_utts(), loudness_groups=DOC_OF, return_levels=True, **kw, **DOC_SERVE)
    got = serving.synthesize_documents(m, _documents(_doc_utts()), **kw, **DOC_SERVE)
    for d, paragraphs in enumerate(_shape(want)):
        assert np.array_equal(got[d], AO.simple_document(paragraphs, 1.0, 0.2, True, m.hp.sampling_rate, IDENT)), d
    ceiling = 10.0 ** (-6.0 / 20.0)
    for d in (0, 1):
        rows = [i for i, k in enumerate(DOC_OF) if k == d]
        tp = max(levels[i]["true_peak"] for i in rows)
        assert all(levels[i]["limited"] for i in rows) and len({levels[i]["gain"] for i in rows}) == 1
        assert abs(levels[rows[0]]["gain"] - ceiling / tp) <= 2.0 ** -23 * levels[rows[0]]["gain"]
    sample = serving.synthesize_documents(m, _documents(_doc_utts()), target_lufs=20.0, peak_ceiling_db=-6.0, as_pcm16=False, **DOC_SERVE)
    assert all(np.abs(a).max() <= np.abs(b).max() for a, b in zip(got, sample))           # the true-peak ceiling is never the looser one
    with pytest.raises(ValueError, match="target_lufs"):
        serving.synthesize_documents(m, _documents(_doc_utts()), peak="true", **DOC_SERVE)
