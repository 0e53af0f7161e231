#!/usr/bin/env python3
"""Timings for the device loudness meter (docs/MEASUREMENTS.md, "Loudness").  GPU only.

    python tools/loudness_bench.py [--calls 200]

At 44.1 kHz, one 4.46 s item (196 608 samples: config 2's utterance) and B = 32 x 10 s (441 000 samples each):

  * ``audio.normalize_loudness(as_pcm16=True)``: the four launches of ``bv2_loudness_measure`` plus the one of ``bv2_loudness_apply``, with
    the wrapper's allocations — what ``serving.synthesize(target_lufs=..., as_pcm16=True)`` adds to a bucket;
  * ``audio.loudness``: the measurement alone;
  * the yardstick: ``serving.pcm16`` (``bv2_pcm16``, the peak-normalising launch the 16-bit path runs without a target) on the same
    waveforms in the same process.

HIP events around ``--calls`` calls after warm-up, median of five runs and the five runs; one JSON line per shape."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bert_vits2_amd import audio, hparams as H, models, serving, synth  # noqa: E402

RATE = 44100
SHAPES = ((1, 196608), (32, 441000))


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/loudness_bench.py needs a GPU")
    dev = torch.cuda.get_device_name(0)
    hp = H.default_v23()
    with torch.device("meta"):                                      # bv2_pcm16 is handle-free: the model only lends serving.pcm16 its library
        m = models.from_hparams(hp)
    for B, S in SHAPES:
        calls = args.calls if B == 1 else max(args.calls // 4, 10)
        base = [synth.synthetic_reference_wav(S, i).float() / 32768 for i in range(4)]
        wav = torch.stack([base[i % 4] for i in range(B)]).cuda()
        lengths = torch.full((B,), S, dtype=torch.int64, device="cuda")
        out, info = audio.normalize_loudness(wav, None, RATE, as_pcm16=True)
        torch.cuda.synchronize()
        row = dict(what="loudness", rate=RATE, B=B, samples=S, seconds=round(S / RATE, 2), lufs_item0=round(float(info["lufs"][0]), 3),
                   calls_per_run=calls, device=dev)
        row["us_normalize_loudness_pcm16"], row["runs_normalize_loudness_pcm16"] = _median_us(
            lambda: audio.normalize_loudness(wav, None, RATE, as_pcm16=True), calls)
        row["us_loudness"], row["runs_loudness"] = _median_us(lambda: audio.loudness(wav, None, RATE), calls)
        row["us_serving_pcm16"], row["runs_serving_pcm16"] = _median_us(lambda: serving.pcm16(m, wav[:, None], lengths, hop=1), calls)
        row["normalize_over_pcm16"] = round(row["us_normalize_loudness_pcm16"] / row["us_serving_pcm16"], 2)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
