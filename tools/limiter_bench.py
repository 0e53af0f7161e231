#!/usr/bin/env python3
"""Timings for the look-ahead true-peak limiter (docs/MEASUREMENTS.md, "Limiter").  GPU only.

    python tools/limiter_bench.py [--calls 200] [--only KEY]

At 44.1 kHz, one 4.46 s item (196 608 samples: config 2's utterance) and a ragged B = 8 batch of up to 30 s (1 323 000 samples), with the
default 3 ms / 60 ms (H = 66, P = 1323):

  * ``audio.limit_apply`` (``bv2_limit``: the envelope launch and the apply launch) under a gain that puts the true peak 6 dB over the
    ceiling (crests: hold and FIR run in the tiles they reach) and under one that leaves it 6 dB below (every tile on the all-pass path);
    the difference of the two is what hold and FIR cost, and ``audio.true_peak_measure`` beside them is the envelope launch's staging and
    tap loop with a fold instead of a store per sample;
  * ``audio.normalize_loudness(limiter=True, makeup_passes=1)`` beside ``peak="true"``, the static path, at a target the ceiling binds on.

``--only KEY`` runs one of the keys a few times without timing, for a kernel trace that splits a call into its launches.  Every figure
includes the wrapper's allocations.  HIP events around ``--calls`` calls after warm-up, median of five runs and the five runs; one JSON
line per shape."""
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
CEILING_DB = -1.0


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
    ap.add_argument("--only", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/limiter_bench.py needs a GPU")
    dev = torch.cuda.get_device_name(0)
    c = 10.0 ** (CEILING_DB / 20.0)
    for B, S in SHAPES:
        calls = args.calls if B == 1 else max(args.calls // 4, 10)
        base = [synth.synthetic_reference_wav(S, i).float() / 32768 for i in range(4)]
        wav = torch.stack([base[i % 4] for i in range(B)]).cuda()
        lens = [S - (b * S) // (2 * B) for b in range(B)]                # ragged: from S down to a bit over S / 2
        wl = torch.tensor(lens, dtype=torch.int64, device="cuda")
        tp = audio.true_peak_measure(wav, wl, RATE)
        over, under = (2.0 * c / tp).float(), (0.5 * c / tp).float()     # the true peak 6 dB over the ceiling, 6 dB under it
        m = audio.loudness_measure(wav, wl, RATE)
        target = float(m["lufs"].max()) + 20.0 * float(torch.log10(over.max()))            # the ceiling binds: the loudest item 6 dB over it
        r = audio.limit_apply(wav, wl, RATE, over, None, CEILING_DB)
        q = audio.limit_apply(wav, wl, RATE, under, None, CEILING_DB)
        out, info = audio.normalize_loudness(wav, wl, RATE, target, CEILING_DB, limiter=True, makeup_passes=1)
        torch.cuda.synchronize()
        assert int(q["limited_samples"].sum()) == 0 and int(r["limited_samples"].min()) > 0
        fns = (("limit_crests", lambda: audio.limit_apply(wav, wl, RATE, over, None, CEILING_DB)),
               ("limit_all_pass", lambda: audio.limit_apply(wav, wl, RATE, under, None, CEILING_DB)),
               ("true_peak", lambda: audio.true_peak_measure(wav, wl, RATE)),
               ("loudness_apply", lambda: audio.loudness_apply(wav, wl, RATE, under)),
               ("normalize_limiter_1", lambda: audio.normalize_loudness(wav, wl, RATE, target, CEILING_DB, limiter=True, makeup_passes=1)),
               ("normalize_limiter_0", lambda: audio.normalize_loudness(wav, wl, RATE, target, CEILING_DB, limiter=True, makeup_passes=0)),
               ("normalize_true", lambda: audio.normalize_loudness(wav, wl, RATE, target, CEILING_DB, peak="true")))
        if args.only:
            for _ in range(5):
                dict(fns)[args.only]()
            torch.cuda.synchronize()
            continue
        row = dict(what="limiter", rate=RATE, B=B, samples=S, seconds=round(S / RATE, 2), plan=audio.limiter_plan(RATE),
                   limited_share_crests=round(float(r["limited_samples"].sum()) / sum(lens), 4),
                   min_gain_db_crests=round(float(audio.min_gain_db(r["min_gain"]).min()), 2), target_lufs=round(target, 2),
                   lufs_out=[round(float(v), 3) for v in info["lufs_out"]], calls_per_run=calls, device=dev)
        for key, fn in fns:
            row["us_" + key], row["runs_" + key] = _median_us(fn, calls)
        row["hold_and_fir_us"] = round(row["us_limit_crests"] - row["us_limit_all_pass"], 2)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
