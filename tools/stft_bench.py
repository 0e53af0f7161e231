#!/usr/bin/env python3
"""Timings for the device spectrogram (docs/MEASUREMENTS.md, "Spectrogram").  GPU only.

    python tools/stft_bench.py [--calls 200] [--seconds 4.6 30]

For spec_channels 1025 / 513 / 80 (``StftParams.from_hparams``), a 4.6 s and a 30 s reference at 44.1 kHz, B = 1 and a ragged B = 8:

  * ``bv2_spectrogram`` with preallocated buffers, in BOTH store layouts — ``frame_major``: [B, L, C] memory handed out as the [B, C, L] view
    (what ``audio.spectrogram`` does), ``channel_major``: contiguous [B, C, L] — with the achieved store bandwidth (the output is the only
    traffic that matters: an int16 waveform is 1 / 1000 of it);
  * ``audio.spectrogram`` as a caller sees it (allocations and the ctypes call included);
  * the yardstick: ``torch.stft`` + the elementwise tail (and the filterbank matmul + log for 80) on the same device and shapes, batch
    padded to the longest item (it has no ragged form).

HIP events around ``--calls`` calls after warm-up, median of five runs; one JSON line per measurement."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bert_vits2_amd import audio, hparams as H, lib as L, synth  # noqa: E402


_WAVS = {}


def _wav(n, i, sr):
    if (n, i, sr) not in _WAVS:
        _WAVS[(n, i, sr)] = synth.synthetic_reference_wav(n, i, sr)
    return _WAVS[(n, i, sr)]


def _timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n


def _median_us(fn, calls):
    for _ in range(20):
        fn()
    torch.cuda.synchronize()
    runs = [1e3 * _timed(fn, calls) for _ in range(5)]
    return round(statistics.median(runs), 2), [round(r, 2) for r in runs]


def _raw_call(p, wav, lengths, layout):
    lib, cfg = L.load(), p.config(L.WAV_I16)
    B, S = wav.shape
    Lf = p.frames(S)
    mem = torch.empty((B, Lf, p.channels) if layout == "frame_major" else (B, p.channels, Lf), dtype=torch.float32, device="cuda")
    spec = mem.transpose(1, 2) if layout == "frame_major" else mem
    strides = (C.c_int64 * 3)(*spec.stride())
    ws = torch.empty(lib.bv2_stft_workspace_bytes(C.byref(cfg), B, S), dtype=torch.uint8, device="cuda")
    n = torch.empty(B, dtype=torch.int64, device="cuda")
    basis = torch.from_numpy(audio.mel_basis(p)).cuda() if p.n_mels else None
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    args = (stream, C.byref(cfg), C.c_void_p(wav.data_ptr()), wav.stride(0), C.c_void_p(lengths.data_ptr()), B, S,
            C.c_void_p(basis.data_ptr()) if basis is not None else None, C.c_void_p(mem.data_ptr()), strides, C.c_void_p(n.data_ptr()),
            C.c_void_p(ws.data_ptr()), ws.numel())

    def call():
        if lib.bv2_spectrogram(*args):
            raise RuntimeError(lib.bv2_last_error(None).decode())
    call.keep = (mem, ws, n, basis, cfg, strides)
    call.spec = spec
    return call


def _torch_yardstick(p, wav):
    wf = wav.float() / 32768
    window = torch.hann_window(p.win, device="cuda")
    basis = torch.from_numpy(audio.mel_basis(p)).cuda() if p.n_mels else None

    def call():
        y = torch.nn.functional.pad(wf[:, None], (p.pad, p.pad), mode="reflect")[:, 0]
        s = torch.stft(y, p.n_fft, hop_length=p.hop, win_length=p.win, window=window, center=False, return_complex=True)
        mag = torch.sqrt(s.real.pow(2) + s.imag.pow(2) + 1e-6)
        return torch.log(torch.clamp(basis @ mag, min=1e-5)) if basis is not None else mag
    return call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--seconds", type=float, nargs="+", default=[4.6, 30.0])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/stft_bench.py needs a GPU")
    dev = torch.cuda.get_device_name(0)
    for spec_channels in (1025, 513, 80):
        p = audio.StftParams.from_hparams(H.default_v23(n_speakers=0, spec_channels=spec_channels))
        for seconds in args.seconds:
            S = int(round(seconds * p.sampling_rate))
            for B in (1, 8):
                lens = [S] if B == 1 else [max(p.min_samples, S * (8 - i) // 8) for i in range(B)]     # ragged: 8/8 .. 1/8 of the longest
                wav = torch.zeros(B, S, dtype=torch.int16)
                for i, n in enumerate(lens):
                    wav[i, :n] = _wav(n, i, p.sampling_rate)
                wav, wl = wav.cuda(), torch.tensor(lens).cuda()
                out_bytes = 4 * p.channels * sum(p.frames(n) for n in lens)                           # live frames only
                row = dict(what="spectrogram", spec_channels=spec_channels, n_fft=p.n_fft, hop=p.hop, n_mels=p.n_mels, seconds=seconds, B=B,
                           frames=p.frames(S), live_output_MB=round(out_bytes / 1e6, 3), calls_per_run=args.calls, device=dev)
                calls = {}
                for layout in ("frame_major", "channel_major"):
                    calls[layout] = _raw_call(p, wav, wl, layout)
                    us, runs = _median_us(calls[layout], args.calls)
                    row[f"us_{layout}"], row[f"runs_{layout}"] = us, runs
                    row[f"store_GBps_{layout}"] = round(out_bytes / us / 1e3, 1)
                torch.cuda.synchronize()
                assert torch.equal(calls["frame_major"].spec, calls["channel_major"].spec)
                row["us_audio_spectrogram"], _ = _median_us(lambda: audio.spectrogram(wav, wl, p), args.calls)
                row["us_torch_stft"], row["runs_torch_stft"] = _median_us(_torch_yardstick(p, wav), args.calls)
                row["torch_over_ours"] = round(row["us_torch_stft"] / row["us_frame_major"], 2)
                print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
