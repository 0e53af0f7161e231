"""CPU: from a waveform to the ReferenceEncoder's spectrogram (kernels/stft.hip, bert_vits2_amd/audio.py) — everything that needs no GPU:
frame arithmetic, the mel filterbank, every refusal of the C ABI (checked before anything touches the device), the parameter objects and
the fixtures' metadata (tests/golden/stft_*.npz, tools/gen_stft_golden.py).  The spectrogram itself runs on the GPU: tests/test_stft_gpu.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from bert_vits2_amd import audio, hparams as H, lib as L, synth
from oracle import mel as oracle_mel
from tests.helpers import GOLDEN, ROOT, load_golden

FIXTURES = ("stft_n2048", "stft_n1024", "stft_ref_enc_wav_g")


def _cfg(n_fft=2048, hop=512, win=None, n_mels=0, fmt=L.WAV_F32):
    c = L.StftConfig()
    c.struct_bytes = C.sizeof(L.StftConfig)
    c.n_fft, c.hop, c.win, c.n_mels, c.input_format = n_fft, hop, n_fft if win is None else win, n_mels, fmt
    return c


def _frames(n_fft, hop, S):
    pad = (n_fft - hop) // 2
    n = S + 2 * pad - n_fft
    return -1 if S <= pad or n < 0 else 1 + n // hop


def test_stft_frames_is_the_formula():
    lib = L.load()
    for n_fft, hop in ((2048, 512), (1024, 256), (1024, 512), (2048, 300), (2048, 2048), (1024, 1)):
        pad = (n_fft - hop) // 2
        for S in (1, pad, pad + 1, pad + 2, n_fft - 2 * pad - 1, n_fft - 2 * pad, 4096, 5000, 12000, 12345, 30000, 44100, 1323000):
            if S < 1:
                continue
            got = lib.bv2_stft_frames(C.byref(_cfg(n_fft, hop)), S)
            assert got == _frames(n_fft, hop, S), (n_fft, hop, S, got)
    # n_fft = 4 hop: S // hop
    for S in (769, 5000, 12345, 44100):
        assert lib.bv2_stft_frames(C.byref(_cfg(2048, 512)), S) == S // 512
    assert lib.bv2_stft_frames(C.byref(_cfg(2048, 512)), 768) < 0
    assert "pad + 1 = 769" in lib.bv2_last_error(None).decode()
    assert lib.bv2_stft_frames(None, 5000) < 0


def test_stft_frames_agree_with_the_fixtures():
    lib = L.load()
    for name in FIXTURES[:2]:
        meta, gold = load_golden(name)
        cfg = _cfg(meta["n_fft"], meta["hop"], meta["win"])
        pad = (meta["n_fft"] - meta["hop"]) // 2
        assert sorted({c["S"] for c in meta["cases"].values()}) == sorted([pad + 1, 5000, 12345])
        for cname, c in meta["cases"].items():
            assert lib.bv2_stft_frames(C.byref(cfg), c["S"]) == c["frames"] == gold[cname + "_spec64"].shape[1], cname
            assert gold[cname + "_spec64"].shape[0] == (meta["n_mels"] if c["n_mels"] else meta["n_fft"] // 2 + 1)
            assert gold[f"wav_s{c['S']}"].dtype == torch.int16 and gold[f"wav_s{c['S']}"].shape == (c["S"],)
    meta, gold = load_golden(FIXTURES[2])
    for cname, c in meta["cases"].items():
        p = audio.StftParams(**c["stft"])
        assert p == audio.StftParams.from_hparams(H.default_v23(n_speakers=0, spec_channels=c["spec_channels"]))
        assert p.frames(c["S"]) == c["frames"] and gold[cname + "_wav"].shape == (c["S"],)


def test_fixture_metadata_is_consistent():
    for name in FIXTURES:
        path = os.path.join(GOLDEN, name + ".npz")
        assert os.path.getsize(path) < 1_000_000, name
        meta, gold = load_golden(name)
        assert "bv2_mel_basis" in meta["mel_note"]
        assert len(meta["cases"]) == (3 if name == FIXTURES[2] else 6)
        for cname, c in meta["cases"].items():
            assert c["ref_err"] > 0 and c["frames"] >= 1, (name, cname)
            key = cname + ("_g64" if name == FIXTURES[2] else "_spec64")
            assert gold[key].dtype == torch.float64 and torch.isfinite(gold[key]).all()
            if name != FIXTURES[2]:
                assert abs(float(gold[key].abs().max()) - c["peak"]) < 1e-9
                # the reference's fp32 error is far below the signal: the bar 4 * ref_err is a real one
                assert c["ref_err"] < 1e-5 * max(c["peak"], 1.0)
            wav = gold[cname + "_wav"] if name == FIXTURES[2] else gold[f"wav_s{c['S']}"]
            assert 0.7 * 32767 <= int(wav.abs().max()) <= 0.8 * 32767 + 1


@pytest.mark.parametrize("sr,n_fft,n_mels,fmin,fmax", [(44100, 2048, 80, 0.0, None), (44100, 1024, 80, 0.0, None),
                                                       (22050, 1024, 80, 50.0, 8000.0)])
def test_mel_basis_is_the_oracles_formula_in_fp64(sr, n_fft, n_mels, fmin, fmax):
    p = audio.StftParams(n_fft, n_fft // 4, n_fft, n_mels, sr, fmin, fmax)
    ours = audio.mel_basis(p, np.float64)
    want = oracle_mel.mel_filterbank(sr, n_fft, n_mels, fmin, fmax)
    assert ours.shape == want.shape == (n_mels, n_fft // 2 + 1)
    err = float(np.abs(ours - want).max())
    print(f"[mel_basis {sr} {n_fft} {n_mels} {fmin} {fmax}] max|ours - oracle| = {err:.3e}  max entry = {float(want.max()):.4f}")
    assert float(want.max()) <= 0.05 and err <= 1e-12
    f32 = audio.mel_basis(p)
    assert f32.dtype == np.float32 and np.array_equal(f32, ours.astype(np.float32))       # rounded once, as the reference rounds librosa's
    nz = (f32 != 0).sum(1)
    assert nz.min() >= 1 and nz.max() < 200                                               # a few dozen non-zeros per row


def _last():
    return L.load().bv2_last_error(None).decode()


def test_every_refusal_names_the_offending_argument():
    lib = L.load()
    bad = [("n_fft", _cfg(512, 128)), ("n_fft", _cfg(4096, 1024)), ("n_fft", _cfg(1000, 250)), ("hop", _cfg(2048, 0)),
           ("hop", _cfg(2048, 2049)), ("win", _cfg(2048, 512, 2049)), ("win", _cfg(2048, 512, 0)), ("n_mels", _cfg(2048, 512, n_mels=-1)),
           ("input_format", _cfg(2048, 512, fmt=7))]
    short = _cfg()
    short.struct_bytes -= 4
    bad.append(("struct_bytes", short))
    dummy = (C.c_float * 16)()                       # never dereferenced: every check precedes the device
    ptr = C.c_void_p(C.addressof(dummy))
    for word, cfg in bad:
        assert lib.bv2_stft_frames(C.byref(cfg), 5000) < 0 and word in _last(), (word, _last())
        assert lib.bv2_stft_workspace_bytes(C.byref(cfg), 1, 5000) < 0 and word in _last(), (word, _last())
        rc = lib.bv2_spectrogram(None, C.byref(cfg), ptr, 5000, None, 1, 5000, None, ptr, None, None, ptr, 1 << 20)
        assert rc != 0 and word in _last(), (word, rc, _last())
        assert lib.bv2_mel_basis(C.byref(cfg), 44100, 0.0, 0.0, ptr) != 0, word
    ok = _cfg(2048, 512, n_mels=80)
    need = lib.bv2_stft_workspace_bytes(C.byref(ok), 1, 5000)
    assert need > 0
    rc = lib.bv2_spectrogram(None, C.byref(ok), ptr, 5000, None, 1, 5000, None, ptr, None, None, ptr, need)
    assert rc != 0 and "mel_basis" in _last(), _last()
    rc = lib.bv2_spectrogram(None, C.byref(ok), ptr, 5000, None, 1, 5000, ptr, ptr, None, None, ptr, 64)
    assert rc != 0 and "workspace" in _last(), _last()
    rc = lib.bv2_spectrogram(None, C.byref(ok), ptr, 5000, None, 1, 5000, ptr, ptr, None, None, None, need)
    assert rc != 0 and "workspace" in _last(), _last()
    rc = lib.bv2_spectrogram(None, C.byref(ok), None, 5000, None, 1, 5000, ptr, ptr, None, None, ptr, need)
    assert rc != 0 and "wav" in _last(), _last()
    rc = lib.bv2_spectrogram(None, C.byref(ok), ptr, 768, None, 1, 768, ptr, ptr, None, None, ptr, need)
    assert rc != 0 and "pad + 1" in _last(), _last()
    rc = lib.bv2_spectrogram(None, C.byref(ok), ptr, 5000, None, 0, 5000, ptr, ptr, None, None, ptr, need)
    assert rc != 0 and "B" in _last(), _last()
    neg = (C.c_int64 * 3)(1025 * 9, -1, 1025)
    rc = lib.bv2_spectrogram(None, C.byref(_cfg()), ptr, 5000, None, 1, 5000, None, ptr, neg, None, ptr, need)
    assert rc != 0 and "spec_strides" in _last(), _last()
    # the same refusals on the Python side
    for kw in (dict(n_fft=512), dict(n_fft=4096), dict(n_fft=1000), dict(hop=0), dict(hop=4096), dict(win=4096), dict(n_mels=-1)):
        with pytest.raises(ValueError, match=next(iter(kw))):
            audio.StftParams(**kw)


def test_stft_params_from_hparams_and_from_config():
    hp = H.default_v23(n_speakers=0, spec_channels=1025)
    assert audio.StftParams.from_hparams(hp) == audio.StftParams(2048, 512, 2048, 0, 44100, 0.0, None)
    assert audio.StftParams.from_hparams(H.default_v23(n_speakers=0, spec_channels=513)) == audio.StftParams(1024, 512, 1024, 0, 44100)
    p80 = audio.StftParams.from_hparams(H.default_v23(n_speakers=0, spec_channels=80))
    assert p80 == audio.StftParams(2048, 512, 2048, 80, 44100, 0.0, None) and p80.channels == 80 and p80.pad == 768
    with pytest.raises(ValueError, match="spec_channels"):
        audio.StftParams.from_hparams(H.default_v23(spec_channels=257))
    # the data block of the reference's configs/config.json
    data = {"training_files": "filelists/train.list", "max_wav_value": 32768.0, "sampling_rate": 44100, "filter_length": 2048, "hop_length": 512,
            "win_length": 2048, "n_mel_channels": 128, "mel_fmin": 0.0, "mel_fmax": None, "n_speakers": 896}
    assert audio.StftParams.from_config({"data": data}) == audio.StftParams(2048, 512, 2048, 0, 44100, 0.0, None)
    assert audio.StftParams.from_config(data, mel=True) == audio.StftParams(2048, 512, 2048, 128, 44100, 0.0, None)
    # nothing of this grew the model's hyper-parameters
    assert not {"filter_length", "win_length", "n_fft", "n_mel_channels"} & {f for f in H.HParams.__dataclass_fields__}


def test_model_carries_its_stft_params():
    from bert_vits2_amd import models
    from oracle import cases
    m = models.from_hparams(H.default_v23(**dict(cases.CASES["narrow_b2_t18"]["hp"], n_speakers=0, spec_channels=513)))
    assert m.stft_params == audio.StftParams(1024, 512, 1024, 0, 44100)
    m.stft_params = audio.StftParams(1024, 256, 800, 0, 44100)
    assert m.stft_params.hop == 256
    with pytest.raises(ValueError, match="spec_channels"):
        m.stft_params = audio.StftParams(2048, 512, 2048)
    table = models.from_hparams(H.default_v23(**cases.CASES["narrow_b2_t18"]["hp"]))
    with pytest.raises(RuntimeError, match="n_speakers=0"):
        table.reference_embedding_from_wav(torch.zeros(5000))


def test_host_side_lengths_are_validated_before_the_device():
    p = audio.StftParams(2048, 512, 2048)
    assert p.pad == 768 and p.min_samples == 769
    with pytest.raises(ValueError, match="pad \\+ 1 = 769"):
        p.frames(768)
    with pytest.raises(ValueError, match="pad \\+ 1 = 769"):
        audio.spectrogram(torch.zeros(768), params=p)
    with pytest.raises(ValueError, match="pad \\+ 1 = 769"):
        audio.spectrogram(torch.zeros(2, 5000), [5000, 768], params=p)
    with pytest.raises(ValueError, match="exceeds"):
        audio.spectrogram(torch.zeros(2, 5000), [5000, 5001], params=p)
    with pytest.raises(ValueError, match="\\[B\\]"):
        audio.spectrogram(torch.zeros(2, 5000), [5000], params=p)
    with pytest.raises(ValueError, match="float32"):
        audio.spectrogram(torch.zeros(5000, dtype=torch.float64), params=p)
    half = audio.StftParams(1024, 512, 1024)          # hop > n_fft / 3: a whole frame is the larger minimum
    assert half.pad == 256 and half.min_samples == 512
    with pytest.raises(ValueError, match="at least 512"):
        half.frames(511)
    assert half.frames(512) == 1


def test_synthetic_reference_wav_is_seeded_and_voice_like():
    a, b = synth.synthetic_reference_wav(12345, 3), synth.synthetic_reference_wav(12345, 3)
    assert a.dtype == torch.int16 and a.shape == (12345,) and torch.equal(a, b)
    assert not torch.equal(a, synth.synthetic_reference_wav(12345, 4))
    assert abs(int(a.abs().max()) - round(0.8 * 32767)) <= 1


def test_new_exports_are_declared_and_the_source_is_built():
    from bert_vits2_amd import build
    assert "kernels/stft.hip" in build.SOURCES
    header = open(os.path.join(ROOT, "include", "bv2.h")).read()
    names = {n for n, *_ in L.SYMBOLS}
    for sym in ("bv2_stft_frames", "bv2_mel_basis", "bv2_mel_basis_f64", "bv2_stft_workspace_bytes", "bv2_spectrogram"):
        assert sym in names and re.search(r"\b%s\(" % sym, header), sym
    assert L.ABI_VERSION == 3 and re.search(r"#define BV2_PACK_LAYOUT 16\b", header)
