"""CPU: the host side of true peak, step energies and loudness range (include/bv2.h bv2_true_peak*, bv2_loudness_steps / _range) and
their numpy oracle (tests/r128_oracle.py): the oversampling plan, the oracle against sines whose true peak and loudness range are known in
closed form (EBU Tech 3341's true-peak window, Tech 3342's +-1 LU), the percentile indices, and every refusal of the new device calls —
made before the device is touched, so they run here without one."""
import ctypes as C
import functools
import math
import os
import re

import numpy as np
import pytest
import torch

from bert_vits2_amd import audio, build, lib as L
from tests import r128_oracle as R
from tests.helpers import ROOT


def err():
    return L.load().bv2_last_error(None).decode()


def cfg_of(rate, fmt=L.WAV_F32):
    return audio.loudness_config(rate, fmt)


# ---- 1. the plan -----------------------------------------------------------------------------------------------------------------------
def test_true_peak_plan():
    lib = L.load()
    for rate, want in ((8000, (4, 36)), (44100, (4, 36)), (48000, (4, 36)), (95999, (4, 36)), (96000, (2, 36)), (191999, (2, 36)),
                       (192000, (1, 0))):
        f, k = C.c_int32(), C.c_int32()
        assert lib.bv2_true_peak_plan(C.byref(cfg_of(rate)), C.byref(f), C.byref(k)) == 0, err()
        assert (f.value, k.value) == want == audio.true_peak_plan(rate), rate
        assert R.factor(rate) == want[0]
        if want[0] > 1:                                        # the table is the resampler's own at rate -> F rate
            assert audio.resample_plan(rate, want[0] * rate) == (want[0], 1, 36)
    assert lib.bv2_true_peak_plan(C.byref(cfg_of(48000)), None, None) == 0
    assert lib.bv2_true_peak_plan(C.byref(cfg_of(7999)), None, None) == -1 and "sample_rate" in err()
    assert lib.bv2_true_peak_plan(C.byref(cfg_of(192001)), None, None) == -1 and "sample_rate" in err()
    bad = cfg_of(48000)
    bad.struct_bytes = 8
    assert lib.bv2_true_peak_plan(C.byref(bad), None, None) == -1 and "struct_bytes" in err()
    assert lib.bv2_true_peak_plan(None, None, None) == -1 and "cfg is null" in err()
    with pytest.raises(ValueError, match="sample_rate"):
        audio.true_peak_plan(7999)
    assert L.TRUE_PEAK_TILE == 1024 and (L.RANGE_SHORT, L.RANGE_SILENT) == (1, 2)


def test_exports_and_sources():
    lib = L.load()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bv2.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(bv2_[a-z0-9_]+)\s*\(", src))
    for name in ("bv2_true_peak_plan", "bv2_true_peak_workspace_bytes", "bv2_true_peak", "bv2_loudness_steps_count", "bv2_loudness_steps",
                 "bv2_loudness_range_workspace_bytes", "bv2_loudness_range"):
        assert name in declared and hasattr(lib, name) and name in [s[0] for s in L.SYMBOLS]
    assert "kernels/truepeak.hip" in build.SOURCES
    assert re.search(r"BV2_TRUE_PEAK_TILE\s*=\s*1024", src) and re.search(r"BV2_RANGE_SHORT\s*=\s*1,\s*BV2_RANGE_SILENT\s*=\s*2", src)


# ---- 2. true peak of faded sines ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def taps64(rate=48000):
    return audio.resample_taps(rate, 4 * rate, np.float64)


# what the closed form gives for (result over the amplitude, sample peak over the amplitude), dB
SINE_READS = ((0.0, 0.0), (0.0, -3.0103), (0.0, -1.2494), (0.0, -0.6877), (0.0, -3.0103), (-0.085, -0.085))


@pytest.mark.parametrize("k", range(len(R.SINES)))
def test_oracle_true_peak_of_a_faded_sine(k):
    amp, f, phase = R.SINES[k]
    x = R.faded_sine(amp, f, phase)
    tp, sp = R.true_peak(x, taps64()), float(np.max(np.abs(x)))
    over, sample = 20 * math.log10(tp / amp), 20 * math.log10(sp / amp)
    print(f"A = {amp}, fs * {f:.4f}, {phase} deg: true peak {over:+.5f} dB of the amplitude, sample peak {sample:+.4f} dB")
    assert R.EBU_TP_WINDOW[0] <= over <= R.EBU_TP_WINDOW[1]
    assert tp >= sp
    want_over, want_sample = SINE_READS[k]
    assert abs(over - want_over) <= (1e-4 if k < 5 else 1e-3) and abs(sample - want_sample) <= 1e-3


def test_oracle_true_peak_edges():
    assert R.true_peak(np.zeros(0), taps64()) == 0.0
    x = np.array([0.25, -0.5, 0.125])
    assert R.true_peak(x) == 0.5                               # F = 1: the sample peak
    y = R.oversample(x, taps64())
    assert y.shape == (4, 3)
    T = taps64()
    want = sum(x[i] * T[2][36 + i - 1] for i in range(3))      # output 1 * 4 + 2: x[1 + jj - 36] T[2][jj]
    assert abs(y[2, 1] - want) <= 1e-15
    assert abs(T[0, 36] - 0.91) <= 1e-5                        # phase 0 is not the identity: the sample peak is taken explicitly


# ---- 3. loudness range of stepped tones ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def range_case(name):
    levels, seconds, want = R.RANGE_CASES[name]
    return R.loudness_range([R.step_energies(R.level_tone(levels, seconds), 8000)], 8000), want


@pytest.mark.parametrize("name", sorted(R.RANGE_CASES))
def test_oracle_loudness_range_of_stepped_tones(name):
    res, want = range_case(name)
    print(f"{name}: LRA {res['lra']:.4f} LU (want {want}), {res['n_kept']} of {res['n_blocks']} blocks, margin {res['margin']:.3e} LU")
    assert abs(res["lra"] - want) <= R.LRA_TOLERANCE
    assert res["margin"] >= R.MARGIN and not res["short"] and not res["silent"]
    if name == "five":
        assert (res["n_kept"], res["n_blocks"]) == (627, 971)
    if name == "40_20":
        assert res["n_kept"] == res["n_blocks"] == 371         # the relative gate keeps the quiet half


def test_oracle_range_flags_and_noise_cases():
    short = R.loudness_range([R.step_energies(R.envelope_noise(0, 2.9), 8000)], 8000)
    assert short["short"] and short["lra"] == 0.0 and short["max_momentary"] == -math.inf and short["n_blocks"] == 0
    silent = R.loudness_range([R.step_energies(np.zeros(4 * 8000), 8000)], 8000)
    assert silent["silent"] and not silent["short"] and silent["lra"] == 0.0 and silent["n_blocks"] == 11
    for seed in (0, 1, 3):
        res = R.loudness_range([R.step_energies(R.envelope_noise(seed), 8000)], 8000)
        assert res["margin"] >= R.MARGIN and res["n_blocks"] == 31 and res["lra"] > 1.0, seed


# ---- 4. percentile indices ---------------------------------------------------------------------------------------------------------------
def test_percentile_indices():
    want = {1: (0, 0), 2: (0, 1), 10: (1, 9), 11: (1, 10), 371: (37, 352)}
    for n, (lo, hi) in want.items():
        assert R.percentile_indices(n) == (lo, hi) == (((n - 1) * 10 + 50) // 100, ((n - 1) * 95 + 50) // 100)
        assert 0 <= lo <= hi < n


# ---- 5. refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals_come_before_the_device():
    """Made-up non-null pointers are never followed: every argument is checked first."""
    lib = L.load()
    p = C.c_void_p(4096)
    good = cfg_of(44100)
    bad_bytes = cfg_of(44100)
    bad_bytes.struct_bytes = 8
    S = 100000
    for c in (cfg_of(7999), bad_bytes, cfg_of(44100, 5)):
        assert lib.bv2_true_peak_workspace_bytes(C.byref(c), 1, S) < 0 and lib.bv2_loudness_range_workspace_bytes(C.byref(c), 1, S) < 0
        assert lib.bv2_loudness_steps_count(C.byref(c), S) < 0
    for B, s in ((0, S), (4097, S), (1, 0)):
        assert lib.bv2_true_peak_workspace_bytes(C.byref(good), B, s) < 0 and lib.bv2_loudness_range_workspace_bytes(C.byref(good), B, s) < 0
    assert lib.bv2_loudness_steps_count(C.byref(good), -1) < 0
    assert lib.bv2_loudness_steps_count(C.byref(good), 4409) == 0 and lib.bv2_loudness_steps_count(C.byref(good), 44100) == 10
    assert audio.loudness_steps_count(8000, 23999) == 29
    need = lib.bv2_true_peak_workspace_bytes(C.byref(good), 2, S)
    assert need >= 2 * -(-S // L.TRUE_PEAK_TILE) * 4

    def tp(cfg=good, taps=p, wav=p, bstride=S, B=2, S=S, out=p, ws=p, nbytes=need):
        return lib.bv2_true_peak(None, C.byref(cfg), taps, wav, bstride, None, B, S, out, ws, nbytes)

    for kw, rc, msg in ((dict(cfg=cfg_of(7999)), -1, "sample_rate"), (dict(cfg=bad_bytes), -1, "struct_bytes"), (dict(wav=None), -1, "wav is null"),
                        (dict(out=None), -1, "peak_out is null"), (dict(taps=None), -1, "taps is null"), (dict(bstride=-1), -1, "wav_bstride"),
                        (dict(B=0), -1, "B must be"), (dict(B=4097), -1, "B must be"), (dict(S=0), -1, "S must be"),
                        (dict(ws=None), -5, "workspace"), (dict(nbytes=need - 257), -5, "workspace")):
        assert tp(**kw) == rc, kw
        assert msg in err(), (kw, err())

    need = lib.bv2_loudness_workspace_bytes(C.byref(good), 2, S)

    def steps(cfg=good, wav=p, bstride=S, B=2, S=S, ss=p, ss_stride=22, peak=None, ms=None, ws=p, nbytes=need):
        return lib.bv2_loudness_steps(None, C.byref(cfg), wav, bstride, None, B, S, ss, ss_stride, peak, ms, ws, nbytes)

    for kw, rc, msg in ((dict(cfg=cfg_of(7999)), -1, "sample_rate"), (dict(wav=None), -1, "wav is null"), (dict(ss=None), -1, "step_ss is null"),
                        (dict(bstride=-1), -1, "wav_bstride"), (dict(B=0), -1, "B must be"), (dict(S=0), -1, "S must be"),
                        (dict(ss_stride=21), -1, "ss_bstride"), (dict(ws=None), -5, "workspace"), (dict(nbytes=need - 257), -5, "workspace")):
        assert steps(**kw) == rc, kw
        assert msg in err(), (kw, err())

    need = lib.bv2_loudness_range_workspace_bytes(C.byref(good), 2, S)

    def rng(cfg=good, ss=p, ss_stride=22, B=2, S=S, groups=None, n_groups=2, lra=p, lo=p, hi=p, st=p, mo=p, flags=p, ws=p, nbytes=need):
        return lib.bv2_loudness_range(None, C.byref(cfg), ss, ss_stride, None, B, S, groups, n_groups, lra, lo, hi, st, mo, flags, ws, nbytes)

    for kw, rc, msg in ((dict(cfg=bad_bytes), -1, "struct_bytes"), (dict(ss=None), -1, "must not be null"), (dict(lra=None), -1, "must not be null"),
                        (dict(flags=None), -1, "must not be null"), (dict(mo=None), -1, "must not be null"), (dict(B=0), -1, "B must be"),
                        (dict(S=0), -1, "S must be"), (dict(n_groups=1), -1, "n_groups"), (dict(groups=p, n_groups=3), -1, "n_groups"),
                        (dict(ss_stride=21), -1, "ss_bstride"), (dict(ws=None), -5, "workspace"), (dict(nbytes=need - 257), -5, "workspace")):
        assert rng(**kw) == rc, kw
        assert msg in err(), (kw, err())


def test_python_wrappers_refuse_before_any_device_call():
    x = torch.zeros(2, 20000)
    with pytest.raises(ValueError, match="sampling rate"):
        audio.true_peak(x)
    with pytest.raises(ValueError, match="sample_rate"):
        audio.true_peak(x, rate=7000)
    with pytest.raises(ValueError, match="float32"):
        audio.true_peak(x.double(), rate=44100)
    with pytest.raises(ValueError, match="outside"):
        audio.true_peak(x, [5, 20001], rate=44100)
    with pytest.raises(ValueError, match="peak must be one of"):
        audio.normalize_loudness(x, rate=44100, peak="rms")
