#!/usr/bin/env python3
"""Timings for the device resampler (docs/MEASUREMENTS.md, "Resampler").  GPU only.

    python tools/resample_bench.py [--calls 200] [--no-synthesize]

For 44.1 -> 48 / 16 / 8 kHz, one 4.46 s item (196 608 samples: config 2's utterance) and B = 32 of them:

  * ``bv2_resample`` with preallocated buffers (fp32 in, the table on the device), with the arithmetic rate it amounts to;
  * the yardstick: the same polyphase filter as ONE ``torch.nn.functional.conv1d`` on the same device in the same process — L output
    channels (channel q holds row (q M) mod L of the same table, shifted by floor(q M / L)), stride M, the [B, L, Q] result interleaved to
    [B, Q L]; its result is compared with ours before it is timed;
  * the ``serving.synthesize`` step at B = 1, config 2's shape (128 symbols, durations pinned to 3 frames per symbol), with and without
    ``output_rate=48000``, host wall-clock per call.

HIP events around ``--calls`` calls after warm-up, median of five runs and the five runs; one JSON line per measurement."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bert_vits2_amd import audio, hparams as H, lib as L, models, serving, synth  # noqa: E402

RATE_IN = 44100
SAMPLES = 196608                                                  # 384 frames x 512: 4.46 s


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


def _raw_call(rate_out, wav):
    lib = L.load()
    B, S = wav.shape
    cfg = audio.resample_config(RATE_IN, rate_out)
    taps = audio.device_taps(RATE_IN, rate_out, wav.device)
    N = audio.resample_length(RATE_IN, rate_out, S)
    dst = torch.empty(B, N, dtype=torch.float32, device=wav.device)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    args = (stream, C.byref(cfg), C.c_void_p(taps.data_ptr()), C.c_void_p(wav.data_ptr()), S, 0, S, None, B, 0, N, C.c_void_p(dst.data_ptr()),
            N, None)

    def call():
        if lib.bv2_resample(*args):
            raise RuntimeError(lib.bv2_last_error(None).decode())
    call.keep, call.out = (cfg, taps), dst
    return call


def _conv1d_yardstick(rate_out, wav):
    Lr, M, K = audio.resample_plan(RATE_IN, rate_out)
    T = torch.from_numpy(audio.resample_taps(RATE_IN, rate_out))
    shift = [(q * M) // Lr for q in range(Lr)]
    width = 2 * K + 1 + max(shift)
    w = torch.zeros(Lr, 1, width)
    for q in range(Lr):
        w[q, 0, shift[q]:shift[q] + 2 * K + 1] = T[(q * M) % Lr]
    w = w.cuda()
    B, S = wav.shape
    N = audio.resample_length(RATE_IN, rate_out, S)
    Q = -(-N // Lr)
    right = (Q - 1) * M + width - K - S

    def call():
        x = torch.nn.functional.pad(wav[:, None], (K, max(right, 0)))
        y = torch.nn.functional.conv1d(x, w, stride=M)                       # [B, L, Q]: output q of block j is sample j L + q
        return y.transpose(1, 2).reshape(B, -1)[:, :N]
    return call


def _synthesize_step(calls):
    hp = H.default_v23()
    m = models.from_hparams(hp)
    m.load_state_dict(synth.synthetic_state_dict(hp, 0, pin_durations=2.5), strict=False)
    m = m.to("cuda").eval()
    b = synth.synthetic_batch([128])
    utt = [serving.Utterance(b["x"][0], b["tone"][0], b["language"][0], b["bert"][0], b["ja_bert"][0], b["en_bert"][0], 3)]
    kw = dict(sdp_ratio=0.0, noise_scale=0.6, noise_scale_w=0.9, length_scale=1.0)
    row = dict(what="serving.synthesize step, B = 1 x 128 symbols, fp32", calls_per_run=calls, device=torch.cuda.get_device_name(0))
    for name, rate in (("model_rate", None), ("output_rate_48000", 48000)):
        for _ in range(5):
            out = serving.synthesize(m, utt, output_rate=rate, **kw)
        runs = []
        for _ in range(5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(calls):
                serving.synthesize(m, utt, output_rate=rate, **kw)
            runs.append(round(1e3 * (time.perf_counter() - t0) / calls, 4))
        row[f"ms_{name}"], row[f"runs_{name}"], row[f"samples_{name}"] = statistics.median(runs), runs, int(out[0].size)
    row["ms_added"] = round(row["ms_output_rate_48000"] - row["ms_model_rate"], 4)
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--no-synthesize", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/resample_bench.py needs a GPU")
    dev = torch.cuda.get_device_name(0)
    for rate_out in (48000, 16000, 8000):
        Lr, M, K = audio.resample_plan(RATE_IN, rate_out)
        for B in (1, 32):
            wav = torch.stack([synth.synthetic_reference_wav(SAMPLES, i % 4).float() / 32768 for i in range(B)]).cuda()
            ours, ref = _raw_call(rate_out, wav), _conv1d_yardstick(rate_out, wav)
            ours()
            torch.cuda.synchronize()
            diff = float((ours.out - ref()).abs().max())
            N = ours.out.shape[1]
            row = dict(what="resample", rate_in=RATE_IN, rate_out=rate_out, L=Lr, M=M, taps=2 * K + 1, B=B, samples_in=SAMPLES, samples_out=N,
                       lane_mapping="four consecutive outputs per lane", max_abs_diff_vs_conv1d=diff, calls_per_run=args.calls, device=dev)
            row["us_bv2_resample"], row["runs_bv2_resample"] = _median_us(ours, args.calls)
            row["GFLOPs_bv2_resample"] = round(2.0 * B * N * (2 * K + 1) / row["us_bv2_resample"] / 1e3, 1)
            row["us_audio_resample"], _ = _median_us(lambda: audio.resample(wav, None, RATE_IN, rate_out), args.calls)
            row["us_torch_conv1d"], row["runs_torch_conv1d"] = _median_us(ref, max(args.calls // 4, 10))
            row["conv1d_over_ours"] = round(row["us_torch_conv1d"] / row["us_bv2_resample"], 2)
            print(json.dumps(row), flush=True)
    if not args.no_synthesize:
        _synthesize_step(max(args.calls // 10, 10))


if __name__ == "__main__":
    main()
