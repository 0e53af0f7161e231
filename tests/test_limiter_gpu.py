"""GPU: the look-ahead true-peak limiter (bv2_limit, kernels/limiter.hip; ``audio.limit``, ``normalize_loudness(limiter=True)``,
``serving.synthesize(limiter=True)``).

The yardstick is tests/limiter_oracle.py.  The envelope is rebuilt on the device from the merged resampler (``audio.resample(x, r, F r)``
and ``|x|``, the way ``composed()`` of tests/test_truepeak_gpu.py does it); from it the oracle's fp32 restatement must give ``curve`` and
``out`` as BITS, in both output formats — lengths around the look-ahead and the kernel's tile, crests at the item's first and last sample,
on either side of a tile boundary and P apart, the reach inside a tile (8 kHz), beyond one (44.1 kHz), F = 2 (96 kHz), H = 1.  Against the
fp64 definition the bar is derived in the oracle (``curve_bound``, ``out_bound``), not tuned.  Then the guarantees of include/bv2.h, the
loudness target that holds, and serving."""
import functools

import numpy as np
import pytest
import torch

from bert_vits2_amd import audio, lib as L, serving
from tests import limiter_oracle as M, r128_oracle as R
from tests.test_resample_gpu import KW, _utts, narrow_model

pytestmark = pytest.mark.gpu

TILE = L.LIMITER_TILE
G = np.float32(1.3)
CEILING_DB = -1.0
C32 = M.ceiling(CEILING_DB)


def bits(t):
    t = t.detach().cpu().contiguous() if isinstance(t, torch.Tensor) else torch.from_numpy(np.array(t))
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def envelope(x, rate):
    """e[i] = max(|x[i]|, max_p |y[i F + p]|) from the resampler's own outputs, on the device; fp32 numpy [n]."""
    x = torch.as_tensor(x)
    n = x.numel()
    F = R.factor(rate)
    e = (x.to(torch.float32) / 32768.0 if x.dtype == torch.int16 else x).abs().cuda()
    if F > 1:
        y, yl = audio.resample(x[None], None, rate, F * rate)
        assert yl.tolist() == [F * n]
        e = torch.maximum(e, y[0, :F * n].abs().view(n, F).amax(1))
    return e.cpu().numpy()


@functools.lru_cache(maxsize=None)
def case(rate, n, times, crests=None, dtype="float32"):
    """One item, its device envelope and the oracle's fp32 restatement — computed once, shared, never changed."""
    H, P = M.plan(rate, *times)
    x = M.crest_signal(n, M.crests(n, P) if crests is None else crests, seed=rate, dtype=dtype)
    want = M.limit32(M.as_f32(x), envelope(x, rate), G, C32, H, P, audio.limiter_window(rate, *times))
    for v in want.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return x, want


def run(x, rate, times, lens=None, **kw):
    return audio.limit(torch.as_tensor(x), lens, rate, gain=float(G), ceiling_db=CEILING_DB, lookahead_ms=times[0], release_ms=times[1],
                       want_curve=True, **kw)


def check_bits(out, info, want, pcm, row=0, n=None):
    n = len(want["curve"]) if n is None else n
    assert torch.equal(bits(info["curve"][row, :n]), bits(want["curve"])), "curve"
    assert torch.equal(bits(out[row, :n]), bits(want["out16"] if pcm else want["out"])), "out"
    assert int(info["limited_samples"][row]) == want["limited_samples"]
    assert torch.equal(bits(info["min_gain"][row:row + 1]), bits(np.array([want["min_gain"]], np.float32)))
    assert not out[row, n:].any() and bool((info["curve"][row, n:] == 1).all())


# ---- 1. bit for bit against the fp32 restatement ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("pcm", [False, True])
@pytest.mark.parametrize("rate", sorted(M.GPU_TIMES))
def test_curve_and_output_bit_for_bit(rate, pcm):
    times = M.GPU_TIMES[rate]
    H, P = M.plan(rate, *times)
    assert audio.limiter_plan(rate, *times) == (H, P, M.GPU_FACTOR[rate], 36)
    for n in M.lengths(H):
        x, want = case(rate, n, times)
        assert want["limited_samples"] > 0
        out, info = run(x, rate, times, as_pcm16=pcm)
        assert out.dtype == (torch.int16 if pcm else torch.float32) and tuple(out.shape) == (1, n)
        check_bits(out, info, want, pcm)
        assert abs(float(info["min_gain_db"][0]) - 20.0 * np.log10(np.float64(want["min_gain"]))) <= 1e-12


@pytest.mark.parametrize("pcm", [False, True])
def test_tiles_on_both_paths_bit_for_bit(pcm):
    """A lone crest in tile 0 of a five-tile item at 8 kHz: the reach lies inside a tile, so the tiles behind it take the all-pass path."""
    rate, times, n = 8000, M.GPU_TIMES[8000], 5 * TILE + 3
    x, want = case(rate, n, times, M.LONE)
    assert 0 < want["limited_samples"] < TILE and np.all(want["curve"][TILE + TILE // 2:] == 1)
    out, info = run(x, rate, times, as_pcm16=pcm)
    check_bits(out, info, want, pcm)


def test_minimum_lookahead_bit_for_bit():
    rate, times = 8000, M.MIN_LOOKAHEAD
    assert audio.limiter_plan(rate, *times)[:2] == (1, 240)
    for n in (1, 2, 3, TILE, 3 * TILE + 17):
        x, want = case(rate, n, times)
        out, info = run(x, rate, times)
        check_bits(out, info, want, False)


# ---- 2. invariance -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", [8000, 44100])
def test_an_item_is_the_same_bits_alone_and_in_any_batch(rate):
    times, n = M.GPU_TIMES[rate], 3 * TILE + 17
    x, want = case(rate, n, times)
    S = 4 * TILE + 100
    big = torch.full((4, S + 333), float("nan"), device="cuda")                 # a batch stride larger than S, NaN padding
    others = (TILE + 1, 2, n, 5)
    for b, m in enumerate(others):
        big[b, :m] = torch.from_numpy(M.crest_signal(m, M.crests(m, 17), seed=b))
    big[2, :n] = torch.from_numpy(x)
    wav = big[:, :S]
    assert wav.stride(0) > S
    out, info = run(wav, rate, times, lens=list(others))
    check_bits(out, info, want, False, row=2, n=n)
    assert bool(torch.isfinite(out).all())                                          # the padding was never read
    # int16 input: x / 32768 is exact, so the float item of the same values gives the same bits
    xi, want_i = case(rate, n, times, dtype="int16")
    out_i, info_i = run(xi, rate, times)
    check_bits(out_i, info_i, want_i, False)
    out_f, info_f = run(M.as_f32(xi), rate, times)
    assert torch.equal(bits(out_i), bits(out_f)) and torch.equal(bits(info_i["curve"]), bits(info_f["curve"]))


# ---- 3. the fp64 definition ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", sorted(M.GPU_TIMES))
def test_curve_and_output_against_the_fp64_oracle(rate):
    times = M.GPU_TIMES[rate]
    H, P = M.plan(rate, *times)
    F = R.factor(rate)
    t64, t32 = audio.resample_taps(rate, F * rate, np.float64), audio.resample_taps(rate, F * rate)
    for n in (2 * H + 1, TILE + 1, 3 * TILE + 17):
        x, _ = case(rate, n, times)
        out, info = run(x, rate, times)
        want = M.limit64(x, G, C32, H, P, t64)
        dc = float(np.max(np.abs(info["curve"][0].cpu().numpy().astype(np.float64) - want["curve"])))
        do = float(np.max(np.abs(out[0].cpu().numpy().astype(np.float64) - want["out"])))
        bc, bo = M.curve_bound(x, G, C32, H, P, t32), M.out_bound(x, G, C32, H, P, t32)
        print(f"rate {rate} n {n}: curve off by {dc:.3e} (bar {bc:.3e}), out off by {do:.3e} (bar {bo:.3e})")
        assert dc <= bc and do <= bo


# ---- 4. the guarantees of include/bv2.h ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", sorted(M.GPU_TIMES))
def test_sample_bound_true_peak_and_counts(rate):
    times = M.GPU_TIMES[rate]
    H, P = M.plan(rate, *times)
    F = R.factor(rate)
    t64, t32 = audio.resample_taps(rate, F * rate, np.float64), audio.resample_taps(rate, F * rate)
    n = 3 * TILE + 17
    x, want = case(rate, n, times)
    out, info = run(x, rate, times)
    assert float(out.abs().max().double()) <= float(C32) * M.SAMPLE_BOUND                      # derived, not measured
    assert int(info["limited_samples"][0]) == want["limited_samples"] == int((info["curve"] < 1).sum())
    assert float(info["min_gain"][0]) == float(info["curve"].min()) == float(want["min_gain"])
    # the output's true peak is measured: the bar is the fp64 oracle's own ratio on the same input plus the interpolation bound
    got = float(audio.true_peak(out, None, rate)[0]) / float(C32)
    ref = R.true_peak(M.limit64(x, G, C32, H, P, t64)["out"], t64) / float(C32)
    bar = ref + R.true_peak_bound(out[0].cpu().numpy(), t32) / float(C32)
    print(f"rate {rate}: output true peak / ceiling {got:.7f} (fp64 oracle {ref:.7f}, bar {bar:.7f})")
    assert got <= bar


@pytest.mark.parametrize("pcm", [False, True])
def test_an_item_under_the_ceiling_is_loudness_apply_bit_for_bit(pcm):
    rate, n = 44100, 3 * TILE + 17
    x = torch.from_numpy(M.crest_signal(n, (), seed=11))[None].cuda()
    gain = torch.tensor([float(G)], device="cuda")
    out, info = audio.limit(x, None, rate, gain=gain, as_pcm16=pcm, want_curve=True)
    assert torch.equal(bits(out), bits(audio.loudness_apply(x, None, rate, gain, None, pcm)))
    assert int(info["limited_samples"][0]) == 0 and float(info["min_gain_db"][0]) == 0.0 and bool((info["curve"] == 1).all())


# ---- 5. the target holds -------------------------------------------------------------------------------------------------------------------
def test_the_loudness_target_holds_under_a_true_peak_ceiling():
    rate, target = 44100, -16.0
    x = torch.from_numpy(M.voiced_bursts())
    static, si = audio.normalize_loudness(x, None, rate, target, CEILING_DB, peak="true")
    landed = float(audio.loudness(static, None, rate)["lufs"][0])
    assert bool(si["limited"][0]) and target - landed >= 2.0
    out, info = audio.normalize_loudness(x, None, rate, target, CEILING_DB, limiter=True, makeup_passes=1)
    fresh = audio.loudness(out, None, rate)["lufs"]
    tp = float(audio.true_peak(out, None, rate)[0]) / float(C32)
    print(f"static path {landed:.3f} LUFS; limiter, one make-up pass {float(fresh[0]):.3f} LUFS, min gain {float(info['min_gain_db'][0]):.2f} dB, "
          f"{int(info['limited_samples'][0])} of {x.numel()} samples limited, output true peak / ceiling {tp:.7f}")
    assert abs(float(fresh[0]) - target) <= 0.5                                                # EBU R128's own tolerance
    assert torch.equal(info["lufs_out"].cpu().view(torch.int64), fresh.cpu().view(torch.int64))
    assert bool(info["limited"][0]) and 0 < int(info["limited_samples"][0]) < x.numel() // 2 and float(info["min_gain_db"][0]) < 0
    assert float(out.abs().max().double()) <= float(C32) * M.SAMPLE_BOUND
    assert float(info["lufs"][0]) == float(si["lufs"][0]) and "true_peak" not in info
    # peak= only selects what info reports; limiter=False is today's call
    out_t, info_t = audio.normalize_loudness(x, None, rate, target, CEILING_DB, limiter=True, makeup_passes=1, peak="true")
    assert torch.equal(bits(out_t), bits(out)) and torch.equal(bits(info_t["true_peak"]), bits(si["true_peak"]))
    off, _ = audio.normalize_loudness(x, None, rate, target, CEILING_DB, peak="true", limiter=False)
    assert torch.equal(bits(off), bits(static))
    # without a make-up pass the output is what one limiter call under the gate's plain gain writes
    out0, info0 = audio.normalize_loudness(x, None, rate, target, CEILING_DB, limiter=True, makeup_passes=0)
    one, _ = audio.limit(x, None, rate, gain=info0["gain"], ceiling_db=CEILING_DB)
    assert torch.equal(bits(out0), bits(one)) and float(info0["lufs_out"][0]) < float(fresh[0])


# ---- 6. serving ----------------------------------------------------------------------------------------------------------------------------
SERVE = dict(max_batch=4, max_pad_ratio=1.5, **KW)
TARGET = -12.0
LOUD = 6.0            # a target no waveform reaches under -1 dBTP by a static gain (peak >= RMS; the K-weighting adds at most 4 dB)


def _seeded(lengths=(17, 24, 9)):
    out = _utts(list(lengths))
    for i, u in enumerate(out):
        u.seed = 3000 + i
    return out


def test_synthesize_without_the_limiter_is_todays_call():
    m = narrow_model()
    for kw in (dict(), dict(target_lufs=TARGET), dict(target_lufs=TARGET, peak="true", loudness_groups=["a", "b", "a"])):
        one = serving.synthesize(m, _seeded(), return_levels=bool(kw), **kw, **SERVE)
        two = serving.synthesize(m, _seeded(), return_levels=bool(kw), limiter=False, lookahead_ms=1.0, release_ms=5.0, makeup_passes=3, **kw,
                                 **SERVE)
        a, b = (one[0], two[0]) if kw else (one, two)
        assert all(np.array_equal(p, q) for p, q in zip(a, b))
        if kw:
            assert one[1] == two[1] and "lufs_out" not in one[1][0]
    with pytest.raises(ValueError, match="target_lufs"):
        serving.synthesize(m, _seeded(), limiter=True, **SERVE)
    with pytest.raises(ValueError, match="makeup_passes"):
        serving.synthesize(m, _seeded(), target_lufs=TARGET, limiter=True, makeup_passes=4, **SERVE)


@pytest.mark.parametrize("groups,output_rate", [(None, None), (["a", "b", "a"], None), (None, 16000), (["a", "b", "a"], 16000)])
def test_synthesize_with_the_limiter_is_normalize_loudness(groups, output_rate):
    m = narrow_model()
    rate = output_rate or m.hp.sampling_rate
    plain = serving.synthesize(m, _seeded(), output_rate=output_rate, **SERVE)
    got, levels = serving.synthesize(m, _seeded(), output_rate=output_rate, target_lufs=LOUD, limiter=True, makeup_passes=1,
                                     loudness_groups=groups, return_levels=True, **SERVE)
    lens = [len(a) for a in plain]
    batch = torch.zeros(len(plain), max(lens))
    for i, a in enumerate(plain):
        batch[i, :len(a)] = torch.from_numpy(a)
    ids = None if groups is None else [sorted(set(groups)).index(k) for k in groups]
    want, info = audio.normalize_loudness(batch, lens, rate, LOUD, -1.0, groups=ids, limiter=True, makeup_passes=1)
    want = want.cpu().numpy()
    for i, (a, lv) in enumerate(zip(got, levels)):
        gi = i if ids is None else ids[i]
        assert np.array_equal(a.view(np.int32), want[i, :lens[i]].view(np.int32)), i
        assert lv["lufs_out"] == float(info["lufs_out"][gi]) and lv["min_gain_db"] == float(info["min_gain_db"][i])
        assert lv["gain"] == float(info["gain"][gi]) and lv["limited"] == bool(info["limited"][gi]) and lv["lufs"] == float(info["lufs"][gi])
        assert lv["limited"] and lv["min_gain_db"] < 0 and float(np.abs(a).max()) <= float(C32) * M.SAMPLE_BOUND
        print(f"utterance {i}: {lv['lufs']:.2f} -> {lv['lufs_out']:.2f} LUFS, min gain {lv['min_gain_db']:.2f} dB, limited {lv['limited']}")
