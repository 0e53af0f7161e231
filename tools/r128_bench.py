#!/usr/bin/env python3
"""Timings for true peak, step energies and loudness range (docs/MEASUREMENTS.md, "True peak and loudness range").  GPU only.

    python tools/r128_bench.py [--calls 200]

At 44.1 kHz, one 4.46 s item (196 608 samples: config 2's utterance) and a ragged B = 8 batch of up to 30 s (1 323 000 samples):

  * ``audio.true_peak_measure`` (``bv2_true_peak``: the fused tile launch and the fold) against the composed path the tree had before it:
    ``audio.resample`` to 4x the rate — the whole oversampled signal written — then ``abs().amax()`` over it and over the samples;
  * ``audio.loudness_steps`` (``bv2_loudness_steps``) beside ``audio.loudness_measure(gate=False)``, the three tile launches they share;
  * ``audio.loudness_range`` (``bv2_loudness_range``) on step energies that are already there;
  * ``audio.normalize_loudness(peak="true")`` beside ``peak="sample"``.

Every figure includes the wrapper's allocations.  HIP events around ``--calls`` calls after warm-up, median of five runs and the five
runs; one JSON line per shape."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bert_vits2_amd import audio, synth  # noqa: E402

RATE = 44100
SHAPES = ((1, 196608), (8, 30 * RATE))


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
        sys.exit("tools/r128_bench.py needs a GPU")
    dev = torch.cuda.get_device_name(0)
    for B, S in SHAPES:
        calls = args.calls if B == 1 else max(args.calls // 4, 10)
        base = [synth.synthetic_reference_wav(S, i).float() / 32768 for i in range(4)]
        wav = torch.stack([base[i % 4] for i in range(B)]).cuda()
        lens = [S - (b * S) // (2 * B) for b in range(B)]                # ragged: from S down to a bit over S / 2
        for b, n in enumerate(lens):
            wav[b, n:] = 0                                              # zeros behind the items: the composed path needs no mask
        wl = torch.tensor(lens, dtype=torch.int64, device="cuda")

        def composed():
            y, _ = audio.resample(wav, wl, RATE, 4 * RATE)
            return torch.maximum(wav.abs().amax(1), y.abs().amax(1))

        tp = audio.true_peak_measure(wav, wl, RATE)
        assert torch.equal(tp, composed())
        steps = audio.loudness_steps(wav, wl, RATE)["step_ss"]
        rng = audio.loudness_range(steps, wl, S, RATE)
        _, info = audio.normalize_loudness(wav, wl, RATE, peak="true")
        torch.cuda.synchronize()
        row = dict(what="r128", rate=RATE, B=B, samples=S, seconds=round(S / RATE, 2), true_peak_item0=round(float(tp[0]), 4),
                   lra_item0=round(float(rng["lra"][0]), 3), calls_per_run=calls, device=dev)
        for key, fn in (("true_peak", lambda: audio.true_peak_measure(wav, wl, RATE)),
                        ("composed_resample_absmax", composed),
                        ("resample_4x_alone", lambda: audio.resample(wav, wl, RATE, 4 * RATE)),
                        ("loudness_steps", lambda: audio.loudness_steps(wav, wl, RATE)),
                        ("loudness_measure_blocks", lambda: audio.loudness_measure(wav, wl, RATE, gate=False)),
                        ("loudness_range", lambda: audio.loudness_range(steps, wl, S, RATE)),
                        ("normalize_true", lambda: audio.normalize_loudness(wav, wl, RATE, peak="true")),
                        ("normalize_sample", lambda: audio.normalize_loudness(wav, wl, RATE))):
            row["us_" + key], row["runs_" + key] = _median_us(fn, calls)
        row["composed_over_true_peak"] = round(row["us_composed_resample_absmax"] / row["us_true_peak"], 2)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
