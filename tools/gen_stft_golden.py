"""Generate ``tests/golden/stft_*.npz``: the REAL reference's waveform -> spectrogram step (``mel_processing.py``) — build-container only.

    python tools/gen_stft_golden.py        # from the repo root, needs the reference checkout (oracle.ref_import)

The reference's ``mel_processing`` is imported from where ``oracle.ref_import`` finds it, with ``librosa.filters`` stubbed in ``sys.modules``
for that import (librosa is not installed): the stub's ``mel`` is the package's own ``bv2_mel_basis``.  The mel cases are therefore the
reference's arithmetic over a REBUILT filterbank, not librosa's (``mel_note`` in the metadata says so; the filterbank itself is held to
``oracle.mel.mel_filterbank`` by tests/test_stft_cpu.py).

``stft_n2048.npz`` / ``stft_n1024.npz``   (n_fft, hop) = (2048, 512) / (1024, 256), win = n_fft, linear and mel-80, for S = pad + 1 (one frame, every
                                        sample of it reflected), 5 000 and 12 345 (not a multiple of hop).  Per case: ``wav`` (int16), ``spec64``
                                        (``spectrogram_torch`` / ``mel_spectrogram_torch`` on ``wav / 32768`` in fp64), and in the metadata
                                        ``ref_err = max|ref_fp32 - ref_fp64|`` — the reference's own fp32 error, what the GPU test's bar is
                                        built from — with the scale (``peak``) and the frame count.
``stft_ref_enc_wav_g.npz``              for spec_channels 1025 / 513 / 80: ``g`` of the chain waveform -> spectrogram -> ReferenceEncoder (the
                                        ``narrow_b2_t18`` model without a speaker table, as tools/gen_ref_enc_golden.py builds it) in fp64, with that
                                        chain's own ``ref_err``; the spectrogram parameters are exactly ``StftParams.from_hparams`` (hop 512 for
                                        every width), S = 12 345.

Waveforms are ``synth.synthetic_reference_wav`` and are STORED: the tests do not regenerate them.
"""
from __future__ import annotations

import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bert_vits2_amd import audio, hparams as H, synth  # noqa: E402
from oracle import cases, ref_import  # noqa: E402

MODEL_CASE = "narrow_b2_t18"
SR = 44100
STFT = ((2048, 512), (1024, 256))
N_MELS = 80
G_SAMPLES = 12345
MEL_NOTE = ("the mel cases are the reference's arithmetic (mel_spectrogram_torch) over the filterbank bv2_mel_basis rebuilds "
            "(librosa.filters.mel defaults: Slaney scale, Slaney norm), not over librosa's own array")


def reference_mel_processing():
    """The reference's mel_processing module, imported in place with ``librosa.filters.mel`` answered by the package's filterbank."""
    if not ref_import.available():
        raise RuntimeError("reference not present at %s" % ref_import.REF)

    def mel(sr, n_fft, n_mels, fmin=0.0, fmax=None):
        return audio.mel_basis(audio.StftParams(n_fft, n_fft // 4, n_fft, n_mels, sr, fmin, fmax))

    librosa, filters = types.ModuleType("librosa"), types.ModuleType("librosa.filters")
    filters.mel = mel
    librosa.filters = filters
    saved = {k: sys.modules.get(k) for k in ("librosa", "librosa.filters")}
    sys.modules["librosa"], sys.modules["librosa.filters"] = librosa, filters
    if ref_import.REF not in sys.path:
        sys.path.insert(0, ref_import.REF)
    try:
        import mel_processing  # noqa: the reference's mel_processing.py
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    return mel_processing


@torch.no_grad()
def reference_spectrogram(mp, wav16: torch.Tensor, p: audio.StftParams, dtype) -> torch.Tensor:
    """[C, L] as the reference computes it from ``audio / max_wav_value`` (data_utils.py:99-138)."""
    mp.mel_basis.clear()          # the reference's cache key leaves n_fft out
    mp.hann_window.clear()
    y = (wav16.to(dtype) / mp.MAX_WAV_VALUE)[None]
    if p.n_mels:
        return mp.mel_spectrogram_torch(y, p.n_fft, p.n_mels, p.sampling_rate, p.hop, p.win, p.fmin, p.fmax, center=False)[0]
    return mp.spectrogram_torch(y, p.n_fft, p.sampling_rate, p.hop, p.win, center=False)[0]


def case_name(S, mel):
    return f"{'mel' if mel else 'lin'}_s{S}"


def model_hparams(spec_channels):
    base = cases.CASES[MODEL_CASE]
    return H.default_v23(**dict(base["hp"], n_speakers=0, spec_channels=spec_channels)), base


def ref_enc_module(hp, sd, dtype=torch.float32):
    mod = ref_import.reference_models().ReferenceEncoder(hp.spec_channels, hp.gin_channels).eval()
    mod.load_state_dict({k[len("ref_enc."):]: v for k, v in sd.items() if k.startswith("ref_enc.")}, strict=True)
    return mod.to(dtype)


def main():
    torch.set_num_threads(1)
    torch.use_deterministic_algorithms(True)
    out_dir = os.path.join(ROOT, "tests", "golden")
    mp = reference_mel_processing()

    for n_fft, hop in STFT:
        arrays, cmeta = {}, {}
        pad = (n_fft - hop) // 2
        for si, S in enumerate((pad + 1, 5000, 12345)):
            wav = synth.synthetic_reference_wav(S, si, SR)
            for mel in (False, True):
                p = audio.StftParams(n_fft, hop, n_fft, N_MELS if mel else 0, SR, 0.0, None)
                s32 = reference_spectrogram(mp, wav, p, torch.float32)
                s64 = reference_spectrogram(mp, wav, p, torch.float64)
                name = case_name(S, mel)
                arrays[name + "_spec64"] = s64.numpy()
                ref_err = float((s32.double() - s64).abs().max())
                cmeta[name] = dict(S=S, index=si, n_mels=p.n_mels, frames=int(s64.shape[1]), ref_err=ref_err, peak=float(s64.abs().max()))
                print(f"n_fft {n_fft} {name}: frames {s64.shape[1]}  ref_err {ref_err:.3e}  peak {float(s64.abs().max()):.2f}")
            arrays[f"wav_s{S}"] = wav.numpy()
        meta = dict(n_fft=n_fft, hop=hop, win=n_fft, sampling_rate=SR, fmin=0.0, fmax=None, n_mels=N_MELS, cases=cmeta, torch=torch.__version__,
                    mel_note=MEL_NOTE, note="spec64 = reference spectrogram_torch / mel_spectrogram_torch in fp64 on wav / 32768; "
                                            "ref_err = max|the same in fp32 - spec64|")
        path = os.path.join(out_dir, f"stft_n{n_fft}.npz")
        np.savez_compressed(path, meta=json.dumps(meta), **arrays)
        print(os.path.basename(path), os.path.getsize(path), "bytes")

    # ---- waveform -> spectrogram -> ReferenceEncoder
    arrays, gmeta = {}, {}
    for i, spec in enumerate((1025, 513, 80)):
        hp, base = model_hparams(spec)
        p = audio.StftParams.from_hparams(hp)
        sd = synth.synthetic_state_dict(hp, base["seed"])
        wav = synth.synthetic_reference_wav(G_SAMPLES, 10 + i, hp.sampling_rate)
        with torch.no_grad():
            y32 = reference_spectrogram(mp, wav, p, torch.float32)[None]
            y64 = reference_spectrogram(mp, wav, p, torch.float64)[None]
            g32 = ref_enc_module(hp, sd)(y32.transpose(1, 2))[0]
            g64 = ref_enc_module(hp, sd, torch.float64)(y64.transpose(1, 2))[0]
        name = f"s{spec}"
        arrays[name + "_wav"] = wav.numpy()
        arrays[name + "_g64"] = g64.numpy()
        ref_err = float((g32.double() - g64).abs().max())
        gmeta[name] = dict(spec_channels=spec, S=G_SAMPLES, index=10 + i, frames=int(y64.shape[2]), ref_err=ref_err,
                           rms=float(g64.pow(2).mean().sqrt()), stft=dict(n_fft=p.n_fft, hop=p.hop, win=p.win, n_mels=p.n_mels,
                                                                          sampling_rate=p.sampling_rate, fmin=p.fmin, fmax=p.fmax))
        print(f"ref_enc_wav_g {name}: frames {y64.shape[2]}  ref_err {ref_err:.3e}  rms {gmeta[name]['rms']:.4f}")
    meta = dict(model_case=MODEL_CASE, seed=cases.CASES[MODEL_CASE]["seed"], cases=gmeta, torch=torch.__version__, mel_note=MEL_NOTE,
                note="g64 = reference spectrogram (StftParams.from_hparams) + ReferenceEncoder in fp64; ref_err = max|the fp32 chain - g64|")
    path = os.path.join(out_dir, "stft_ref_enc_wav_g.npz")
    np.savez_compressed(path, meta=json.dumps(meta), **arrays)
    print(os.path.basename(path), os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
