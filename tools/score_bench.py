#!/usr/bin/env python3
"""Timings for scoring a take (docs/MEASUREMENTS.md, "Scoring a take").  GPU only.

    python tools/score_bench.py [--calls 50]
    python tools/score_bench.py --trace-calls N --what duration_nll     # setup + N calls of one entry and nothing else: run it under a kernel
                                                                        # tracer with N = 1 and N = 3; (count_3 - count_1) / 2 is the launches of
                                                                        # one call (B = 1 shape), setup and warm-up cancel

The two shapes of tools/align_bench.py (B = 1, a 4.6 s recording against 100 symbols; a ragged B = 8 of 30 s recordings against up to 512
symbols), the default v2.3 model with synthetic weights.  Per shape, HIP events around ``--calls`` calls after warm-up (median of five
runs): ``duration_nll`` (35 launches), ``align.kl_path`` (2), and ``net_g.score`` beside ``net_g.align`` on the same inputs.  One JSON line
per measurement."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bert_vits2_amd import align, hparams as H, models, synth  # noqa: E402
from align_bench import SHAPES, _median_us  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--trace-calls", type=int, default=0)
    ap.add_argument("--what", default="duration_nll", choices=["duration_nll", "kl_path", "score"])
    a = ap.parse_args()
    hp = H.default_v23()
    m = models.from_hparams(hp)
    m.load_state_dict(synth.synthetic_state_dict(hp, 0), strict=False)
    m = m.to("cuda").eval()
    m.load_posterior(synth.synthetic_posterior_state_dict(hp, 0))
    m.load_sdp_forward(synth.synthetic_sdp_forward_state_dict(hp, 0))
    for name, sh in SHAPES.items():
        xl, yl = sh["x"], sh["y"]
        B, T, Ty = len(xl), max(xl), max(yl)
        batch = synth.synthetic_batch(xl, languages=[i % 3 for i in range(B)], sids=list(range(B)))
        dev = lambda k: batch[k].cuda()
        y = torch.rand(B, hp.spec_channels, Ty, generator=torch.Generator().manual_seed(1)).cuda()
        yl_d, xl_d = torch.tensor(yl).cuda(), torch.tensor(xl).cuda()
        args = (dev("x"), xl_d, dev("sid"), dev("tone"), dev("language"), dev("bert"), dev("ja_bert"), dev("en_bert"), y, yl_d)
        out = m.score(*args)
        ne = torch.randn(B, 2, T).cuda()
        enc, post, z_p, dur = out["enc"], out["posterior"], out["z_p"], out["durations"]
        rows = [
            ("duration_nll", lambda: m.duration_nll(enc, dur, noise_e=ne), 35),
            ("kl_path", lambda: align.kl_path(z_p, post["logs_q"], enc["m_p"], enc["logs_p"], dur, xl_d, yl_d), 2),
            ("align", lambda: m.align(*args), None),
            ("score", lambda: m.score(*args, noise_e=ne), None),
        ]
        if a.trace_calls:
            fn = dict((r[0], r[1]) for r in rows)[a.what]
            torch.cuda.synchronize()
            for _ in range(a.trace_calls):
                fn()
            torch.cuda.synchronize()
            print(json.dumps(dict(shape=name, what=a.what, traced_calls=a.trace_calls)), flush=True)
            break
        for what, fn, launches in rows:
            calls = max(5, a.calls // (8 if B > 1 else 1))
            med, runs = _median_us(fn, calls)
            print(json.dumps(dict(shape=name, B=B, T=T, Ty=Ty, what=what, median_us=med, runs_us=runs, launches=launches)), flush=True)


if __name__ == "__main__":
    main()
