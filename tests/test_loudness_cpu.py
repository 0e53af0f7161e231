"""CPU: the host side of the loudness meter (include/bv2.h bv2_loudness_*) and its numpy oracle (tests/loudness_oracle.py): the K-weighting
coefficients against the table of ITU-R BS.1770-4, the oracle against the standard's tone levels and its relative gate, the block
arithmetic, and every refusal of the device calls — made before the device is touched, so they run here without one."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

from bert_vits2_amd import audio, build, lib as L
from tests import loudness_oracle as O
from tests.helpers import ROOT

RATES = (48000, 44100, 24000, 16000, 8000)


def err():
    return L.load().bv2_last_error(None).decode()


def cfg_of(rate, fmt=L.WAV_F32):
    return audio.loudness_config(rate, fmt)


def tone(level_lufs, seconds, rate, f=997.0, phase=0.0):
    """A sine that reads ``level_lufs``: a 997 Hz tone of amplitude A reads -3.01 + 20 log10 A (BS.1770: 0 dBFS gives -3.01 LKFS)."""
    A = 10.0 ** ((level_lufs + 3.01) / 20.0)
    return A * np.sin(2 * np.pi * f * np.arange(int(seconds * rate)) / rate + phase)


def test_coefficients_at_48k_are_the_standards_table():
    c = audio.loudness_coeffs(48000)
    want = list(O.BS1770_48K["b"]) + list(O.BS1770_48K["a1"]) + list(O.BS1770_48K["a2"])
    got = list(c[:5]) + list(c[8:])
    d = max(abs(a - b) for a, b in zip(got, want))
    print(f"48 kHz: max |coeff - table| = {d:.3e}")
    assert d <= 1e-12
    assert list(c[5:8]) == [1.0, -2.0, 1.0]


@pytest.mark.parametrize("rate", RATES[1:])
def test_coefficients_follow_the_bilinear_form(rate):
    c, want = audio.loudness_coeffs(rate), O.coeffs(rate)
    d = np.max(np.abs(c - want) / np.abs(want))
    print(f"{rate}: max relative difference {d:.3e}")
    assert d <= 1e-12


@pytest.mark.parametrize("rate", RATES)
def test_oracle_reads_a_997_hz_sine(rate):
    """EBU Tech 3341's tolerance: 0.1 LU."""
    for A in (1.0, 0.1):
        x = A * np.sin(2 * np.pi * 997.0 * np.arange(3 * rate) / rate)
        got = O.measure([x], rate)["lufs"]
        print(f"{rate} Hz, A = {A}: {got:.4f} (want {-3.01 + 20 * math.log10(A):.4f})")
        assert abs(got - (-3.01 + 20 * math.log10(A))) <= 0.1


def test_oracle_relative_gate_on_the_tone_sequence():
    """-36 / -23 / -36 LUFS for 10 s + 60 s + 10 s (EBU Tech 3341, case 3): the -36 parts fall below the relative gate and the reading is
    -23.  Without the relative gate it would be -23 + 10 log10((60 + 20 * 10^-1.3) / 80) = -24.18."""
    rate = 48000
    x = np.concatenate([tone(-36, 10, rate), tone(-23, 60, rate), tone(-36, 10, rate)])
    res = O.measure([x], rate)
    print(f"tone sequence: {res['lufs']:.4f} LUFS, relative threshold {res['rel_threshold']:.3f}")
    assert abs(res["lufs"] + 23.0) <= 0.1
    l = -0.691 + 10 * np.log10(res["block_ms"][0])
    assert (l <= res["rel_threshold"]).sum() > 150 and (l > res["rel_threshold"]).sum() > 550


@pytest.mark.parametrize("rate", RATES + (22050, 96000, 192000))
def test_plan_and_block_counts(rate):
    lib = L.load()
    step, block, tile = audio.loudness_plan(rate)
    assert (step, block) == O.plan(rate) == (int(round(rate / 10)), 4 * int(round(rate / 10)))
    assert tile >= 256 and (tile - 1) // step + 2 <= 8              # the steps a tile can touch fit the kernel's partial sums
    cfg = cfg_of(rate)
    for n, want in ((0, 0), (1, 1), (block - 1, 1), (block, 1), (block + step - 1, 1), (block + step, 2), (10 * block + 3, 37)):
        assert lib.bv2_loudness_blocks(C.byref(cfg), n) == want == O.n_blocks(n, rate) == audio.loudness_blocks(rate, n)
    assert lib.bv2_loudness_blocks(C.byref(cfg), -1) < 0
    assert lib.bv2_loudness_workspace_bytes(C.byref(cfg), 4, 3 * tile) > 0


def test_refusals_come_before_the_device():
    """Made-up non-null pointers are never followed: every argument is checked first."""
    lib = L.load()
    p = C.c_void_p(4096)
    good = cfg_of(44100)
    bad_bytes = cfg_of(44100)
    bad_bytes.struct_bytes = 8
    v = [C.c_int32() for _ in range(3)]
    for c, msg in ((cfg_of(7999), "sample_rate"), (cfg_of(192001), "sample_rate"), (cfg_of(0), "sample_rate"), (bad_bytes, "struct_bytes"),
                   (cfg_of(44100, 5), "input_format")):
        assert lib.bv2_loudness_plan(C.byref(c), *[C.byref(x) for x in v]) == -1 and msg in err()
        assert lib.bv2_loudness_coeffs(C.byref(c), p) == -1 and msg in err()
        assert lib.bv2_loudness_blocks(C.byref(c), 10) < 0 and lib.bv2_loudness_workspace_bytes(C.byref(c), 1, 10) < 0
    assert lib.bv2_loudness_plan(None, None, None, None) == -1 and "cfg is null" in err()
    assert lib.bv2_loudness_coeffs(C.byref(good), None) == -1 and "out is null" in err()
    assert lib.bv2_loudness_workspace_bytes(C.byref(good), 0, 10) < 0 and lib.bv2_loudness_workspace_bytes(C.byref(good), 1, 0) < 0
    assert lib.bv2_loudness_workspace_bytes(C.byref(good), 4097, 10) < 0 and "4096" in err()

    S = 10000
    need = lib.bv2_loudness_workspace_bytes(C.byref(good), 2, S)

    def measure(cfg=good, wav=p, B=2, S=S, groups=None, n_groups=2, lufs=p, gain=p, peak=p, flags=p, block_ms=None, ws=p, nbytes=need,
                target=-23.0, ceiling=-1.0, bstride=S):
        return lib.bv2_loudness_measure(None, C.byref(cfg), wav, bstride, None, B, S, groups, n_groups, target, ceiling, lufs, gain, peak,
                                        flags, block_ms, ws, nbytes)

    for kw, rc, msg in ((dict(cfg=cfg_of(7999)), -1, "sample_rate"), (dict(cfg=bad_bytes), -1, "struct_bytes"), (dict(wav=None), -1, "wav is null"),
                        (dict(peak=None), -1, "peak is null"), (dict(lufs=None), -1, "go together"), (dict(flags=None), -1, "go together"),
                        (dict(lufs=None, gain=None, flags=None), -1, "block_ms is null"), (dict(B=0), -1, "B must be"),
                        (dict(B=4097, n_groups=4097), -1, "B must be"), (dict(S=0), -1, "S must be"), (dict(n_groups=1), -1, "n_groups"),
                        (dict(groups=p, n_groups=3), -1, "n_groups"), (dict(groups=p, n_groups=0), -1, "n_groups"),
                        (dict(bstride=-1), -1, "wav_bstride"), (dict(target=float("nan")), -1, "finite"),
                        (dict(ceiling=float("inf")), -1, "finite"), (dict(ws=None), -5, "workspace"), (dict(nbytes=need - 257), -5, "workspace")):
        assert measure(**kw) == rc, kw
        assert msg in err(), (kw, err())

    def gate(cfg=good, ms=p, bstride=100, B=2, S=S, peak=p, groups=None, n_groups=2, lufs=p, gain=p, flags=p, ws=p, nbytes=1024):
        return lib.bv2_loudness_gate(None, C.byref(cfg), ms, bstride, None, B, S, peak, groups, n_groups, -23.0, -1.0, lufs, gain, flags, ws,
                                     nbytes)

    for kw, rc, msg in ((dict(cfg=cfg_of(500000)), -1, "sample_rate"), (dict(ms=None), -1, "must not be null"), (dict(peak=None), -1, "must not be null"),
                        (dict(gain=None), -1, "must not be null"), (dict(B=0), -1, "B must be"), (dict(n_groups=3), -1, "n_groups"),
                        (dict(ws=None), -5, "workspace"), (dict(nbytes=63), -5, "workspace"), (dict(S=17640 * 4, bstride=3), -1, "ms_bstride")):
        assert gate(**kw) == rc, kw
        assert msg in err(), (kw, err())

    def apply(cfg=good, src=p, B=2, S=S, groups=None, n_groups=2, gain=p, f32=p, i16=None, dstride=S, sstride=S):
        return lib.bv2_loudness_apply(None, C.byref(cfg), src, sstride, None, B, S, groups, n_groups, gain, f32, i16, dstride)

    for kw, msg in ((dict(cfg=bad_bytes), "struct_bytes"), (dict(cfg=cfg_of(100)), "sample_rate"), (dict(src=None), "src is null"),
                    (dict(gain=None), "gain is null"), (dict(i16=p), "exactly one"), (dict(f32=None), "exactly one"), (dict(B=0), "B must be"),
                    (dict(B=65536, n_groups=65536), "B must be"), (dict(S=0), "S must be"), (dict(n_groups=1), "n_groups"),
                    (dict(groups=p, n_groups=0), "n_groups"),
                    (dict(dstride=S - 1), "dst_bstride"), (dict(sstride=-1), "src_bstride")):
        assert apply(**kw) == -1, kw
        assert msg in err(), (kw, err())


def test_abi_version_exports_and_sources():
    lib = L.load()
    assert lib.bv2_abi_version() == 3 == L.ABI_VERSION
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bv2.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(bv2_[a-z0-9_]+)\s*\(", src))
    for name in ("bv2_loudness_plan", "bv2_loudness_coeffs", "bv2_loudness_blocks", "bv2_loudness_workspace_bytes", "bv2_loudness_measure",
                 "bv2_loudness_gate", "bv2_loudness_apply"):
        assert name in declared and hasattr(lib, name) and name in [s[0] for s in L.SYMBOLS]
    assert C.sizeof(L.LoudnessConfig) == 12
    assert "kernels/loudness.hip" in build.SOURCES
    assert (L.LOUDNESS_SILENT, L.LOUDNESS_LIMITED) == (1, 2)


def test_python_wrappers_refuse_before_any_device_call():
    x = torch.zeros(2, 20000)
    for fn in (audio.loudness, audio.normalize_loudness):
        with pytest.raises(ValueError, match="sampling rate"):
            fn(x)
        with pytest.raises(ValueError, match="sample_rate"):
            fn(x, rate=7000)
        with pytest.raises(ValueError, match=r"\[B, S\]"):
            fn(torch.zeros(2, 3, 4), rate=44100)
        with pytest.raises(ValueError, match=r"\[B, S\]"):
            fn(torch.zeros(2, 0), rate=44100)
        with pytest.raises(ValueError, match="float32"):
            fn(x.double(), rate=44100)
        with pytest.raises(ValueError, match="float32"):
            fn(x.to(torch.int32), rate=44100)
        with pytest.raises(ValueError, match=r"wav_lengths must be \[B\]"):
            fn(x, [5, 6, 7], rate=44100)
        with pytest.raises(ValueError, match="outside"):
            fn(x, [5, 20001], rate=44100)
        with pytest.raises(ValueError, match="outside"):
            fn(x, [0, 5], rate=44100)
        with pytest.raises(ValueError, match=r"groups must be \[B\]"):
            fn(x, rate=44100, groups=[0])
        with pytest.raises(ValueError, match="group ids"):
            fn(x, rate=44100, groups=[0, 2])
        with pytest.raises(ValueError, match="group ids"):
            fn(x, rate=44100, groups=[-1, 0])
    with pytest.raises(ValueError, match="finite"):
        audio.normalize_loudness(x, rate=44100, target_lufs=float("nan"))
