#!/usr/bin/env python3
"""What per-utterance noise seeds cost or save (docs/MEASUREMENTS.md, "Seeded noise").  GPU only.

    python tools/seeded_noise_bench.py [--steps 40] [--rounds 7]

A/B in ONE process: the drawn path (``infer(...)``: ``draw_noise_w`` / ``draw_noise_z`` from torch's generators, the behaviour without
seeds and the BASELINE) against the seeded path (``infer(..., seeds=...)``: the noise computed inside ``front_kernel`` and the expand role
of ``phase_b_front_kernel``).  The two alternate round by round — drawn, seeded, drawn, ... — so that drift of the box lands on both;
each round times ``--steps`` steps between two device synchronisations with the host clock.  Reported per configuration: the median
round of each path, the spread (max - min) / min of each path's rounds, and seeded / drawn.

  * config 2's shape: B = 1 x 128 symbols, fp32, durations pinned to 3 frames per symbol (T_y = 384); eager, then hipGraph replay;
  * config 3's shape: B = 32 x 128 symbols, bf16 Generator + fp16 flow, hipGraph replay with ``ty_bucket=32``;
  * ``phase_b_front`` alone: the library's per-launch HIP events (``model.profile(3)``, eager), both shapes.

``sdp_ratio`` is 0.5 here (bench.py's configs run at 0, where the stochastic predictor and its noise are skipped by both paths): the
front kernel's share of the change is then inside the step.  Both paths get ``w_ceil`` = 3 frames per symbol after phase A, so every
step of both runs at T_y = 384 whatever the stochastic predictor drew.  One JSON line per measurement."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bert_vits2_amd import hparams as H, models, synth  # noqa: E402

KW = dict(noise_scale=0.6, noise_scale_w=0.9, sdp_ratio=0.5, length_scale=1.0)
ARGS = ("x", "x_lengths", "sid", "tone", "language", "bert", "ja_bert", "en_bert")


def _round_ms(call, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        call()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def _ab(calls, steps, rounds, warmup=5):
    for c in calls.values():
        for _ in range(warmup):
            c()
    torch.cuda.synchronize()
    ms = {k: [] for k in calls}
    for _ in range(rounds):
        for k, c in calls.items():                     # alternate inside every round
            ms[k].append(_round_ms(c, steps))
    out = {}
    for k, v in ms.items():
        out[f"{k}_ms_median"] = round(statistics.median(v), 4)
        out[f"{k}_ms_rounds"] = [round(x, 4) for x in v]
        out[f"{k}_spread"] = round((max(v) - min(v)) / min(v), 4)
    out["seeded_over_drawn"] = round(out["seeded_ms_median"] / out["drawn_ms_median"], 4)
    return out


def _front_row(model, call, steps):
    model.profile(3)
    for _ in range(steps):
        call()
    torch.cuda.synchronize()
    rows = [r for r in model.profile_report() if r["name"].startswith("phase_b_front")]
    model.profile(0)
    n = sum(r["launches"] for r in rows)
    return round(1e3 * sum(r["total_ms"] for r in rows) / max(n, 1), 2), n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/seeded_noise_bench.py needs a GPU")
    dev = torch.device("cuda")
    hp = H.default_v23()
    model = models.from_hparams(hp)
    model.load_state_dict(synth.synthetic_state_dict(hp, seed=0, pin_durations=2.5), strict=False)
    model = model.to(dev).eval()
    name = torch.cuda.get_device_name(0)
    for cfg, B, gen, flow, modes in ((2, 1, torch.float32, torch.float32, ("eager", "graphs")),
                                     (3, 32, torch.bfloat16, torch.float16, ("graphs",))):
        model.enable_graphs(False)
        model.set_generator_dtype(gen)
        model.set_flow_dtype(flow)
        batch = {k: v.to(dev) for k, v in synth.synthetic_batch([128] * B).items()}
        seeds = torch.arange(1, B + 1, dtype=torch.int64, device=dev)
        wc = torch.full((B, 128), 3.0, device=dev)      # both paths at the same T_y = 384 whatever the SDP draws (infer(w_ceil=...))
        calls = dict(drawn=lambda: model.infer(*[batch[k] for k in ARGS], w_ceil=wc, **KW),
                     seeded=lambda: model.infer(*[batch[k] for k in ARGS], w_ceil=wc, seeds=seeds, **KW))
        steps = args.steps if B == 1 else max(5, args.steps // 4)
        for mode in modes:
            model.enable_graphs(mode == "graphs", static_io=True, ty_bucket=32)
            row = dict(what="step", config_shape=cfg, B=B, T=128, mode=mode, generator=str(gen).split(".")[1], flow=str(flow).split(".")[1],
                       sdp_ratio=KW["sdp_ratio"], steps_per_round=steps, rounds=args.rounds, device=name)
            row.update(_ab(calls, steps, args.rounds))
            row["Ty"] = int(calls["seeded"]()[2].shape[2])
            print(json.dumps(row), flush=True)
        model.enable_graphs(False)
        row = dict(what="phase_b_front", config_shape=cfg, B=B, Ty=row["Ty"], source="per-launch HIP events (profile mode 3), eager", device=name)
        for _ in range(5):                             # drawn, seeded, drawn, seeded, ...: the mean of each pass's launches
            for k, c in calls.items():
                us, n = _front_row(model, c, 60 if B == 1 else 15)
                row.setdefault(f"{k}_us", []).append(us)
                row[f"{k}_launches"] = n
        for k in calls:
            row[f"{k}_us_median"] = statistics.median(row[f"{k}_us"])
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
