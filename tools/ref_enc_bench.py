#!/usr/bin/env python3
"""Timings for speaker conditioning from a reference spectrogram / a given vector (docs/MEASUREMENTS.md, "ReferenceEncoder").  GPU only.

    python tools/ref_enc_bench.py embed [--calls 300]      reference_embedding at B = 1, spec 1025, L = 400 and L = 96: time per call
    python tools/ref_enc_bench.py given_g [--steps 40]     config 2 (B = 1, T = 128, fp32) and config 3 (B = 32 x 128, bf16 Generator, fp16
                                                           flow, hipGraph replay), infer(sid=...) against infer(g=...), same process,
                                                           alternating blocks
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/ref_enc_bench.py embed --calls 20 --profile
                                                           the per-kernel split and the launch count (a run of its own: tracing slows the host)

Every figure is a device-event time around work that ends in a synchronise; one JSON line per measurement."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bert_vits2_amd import hparams as H, models, synth  # noqa: E402


def _model(hp, **kw):
    m = models.from_hparams(hp)
    m.load_state_dict(synth.synthetic_state_dict(hp, 0, **kw), strict=False)
    return m.to("cuda").eval()


def _timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n


def embed(args):
    m = _model(H.default_v23(n_speakers=0))
    for L in (400, 96):
        y = synth.synthetic_reference_spec(1025, L, 0)[None].cuda()
        for _ in range(3 if args.profile else 20):
            m.reference_embedding(y)
        torch.cuda.synchronize()
        if args.profile:
            for _ in range(args.calls):
                m.reference_embedding(y)
            torch.cuda.synchronize()
            continue
        per = [_timed(lambda: m.reference_embedding(y), args.calls) for _ in range(5)]
        print(json.dumps(dict(what="reference_embedding", B=1, spec_channels=1025, L=L, gin=m.hp.gin_channels, launches_per_call=8,
                              us_per_call_median=round(1e3 * statistics.median(per), 2), us_per_call_runs=[round(1e3 * p, 2) for p in per],
                              calls_per_run=args.calls, device=torch.cuda.get_device_name(0))))


def given_g(args):
    hp = H.default_v23()
    m = _model(hp, pin_durations=2.5)
    for name, B, T in (("config2", 1, 128), ("config3", 32, 128)):
        if name == "config3":
            m.set_generator_dtype(torch.bfloat16)
            m.set_flow_dtype(torch.float16)
            m.enable_graphs(True, static_io=True)
        batch = synth.synthetic_batch([T] * B, [i % 3 for i in range(B)], [(7 * i) % hp.n_speakers for i in range(B)])
        a = [batch[k].cuda() for k in ("x", "x_lengths", "sid", "tone", "language", "bert", "ja_bert", "en_bert")]
        g = m.stage_emb_g(a[2])
        kw = dict(noise_scale=0.6, noise_scale_w=0.9, sdp_ratio=0.0, length_scale=1.0, want_attn=False)
        runs = dict(sid=lambda: m.infer(*a, **kw), g=lambda: m.infer(*a, g=g, **kw))
        for fn in runs.values():
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        ms = dict(sid=[], g=[])
        for _ in range(args.blocks):                       # alternating blocks in one process
            for k, fn in runs.items():
                ms[k].append(_timed(fn, args.steps))
        med = {k: statistics.median(v) for k, v in ms.items()}
        print(json.dumps(dict(what=f"{name}: infer(sid) vs infer(g)", B=B, T=T, steps_per_block=args.steps, blocks=args.blocks,
                              ms_per_step_sid=round(med["sid"], 4), ms_per_step_g=round(med["g"], 4),
                              g_over_sid=round(med["g"] / med["sid"], 4), sid_blocks=[round(v, 4) for v in ms["sid"]],
                              g_blocks=[round(v, 4) for v in ms["g"]], device=torch.cuda.get_device_name(0))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["embed", "given_g"])
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--profile", action="store_true", help="no timing, just the calls (for a kernel trace)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/ref_enc_bench.py needs a GPU")
    torch.manual_seed(0)
    {"embed": embed, "given_g": given_g}[args.mode](args)


if __name__ == "__main__":
    main()
