#!/usr/bin/env python3
"""Timings for forced alignment (docs/MEASUREMENTS.md, "Forced alignment").  GPU only.

    python tools/align_bench.py [--calls 50]
    python tools/align_bench.py --shape b1_4.6s_100sym --trace-calls N     # setup + N calls of net_g.align and nothing else: run it under a
                                                                           # kernel tracer with N = 1 and N = 3; (count_3 - count_1) / 2 is
                                                                           # the launches of one align, setup and warm-up cancel

Two shapes, the default v2.3 model with synthetic weights and seeded-noise latents (the kernels' time does not depend on the values):

  * B = 1, a 4.6 s recording (396 frames at hop 512 / 44.1 kHz) against 100 symbols;
  * a ragged B = 8 of 30 s recordings (2584 frames the longest) against up to 512 symbols.

Per shape, HIP events around ``--calls`` calls after warm-up (median of five runs): phase A (the text's prior), the posterior encoder
(``posterior_encode``), the forward flow (``stage_flow_forward``), ``neg_cent``, ``maximum_path`` with and without the one-hot ``attn``,
``align_latent`` and the whole of ``net_g.align`` (spectrogram in, durations out, phase A included); and what a row of the
dynamic programme costs (the ``maximum_path`` time over the longest item's frames: the rows of a workgroup run in sequence, and the
workgroups of a batch side by side).  One JSON line per measurement."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bert_vits2_amd import align, hparams as H, models, synth  # noqa: E402

SHAPES = {
    "b1_4.6s_100sym": dict(x=[100], y=[396]),
    "b8_30s_ragged": dict(x=[512, 470, 433, 401, 377, 350, 322, 300], y=[2584, 2400, 2300, 2100, 2000, 1900, 1700, 1600]),
}


def _timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n


def _median_us(fn, calls):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    runs = [1e3 * _timed(fn, calls) for _ in range(5)]
    return round(statistics.median(runs), 1), [round(r, 1) for r in runs]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--shape", default=None, choices=sorted(SHAPES))
    ap.add_argument("--trace-calls", type=int, default=0)
    a = ap.parse_args()
    hp = H.default_v23()
    m = models.from_hparams(hp)
    m.load_state_dict(synth.synthetic_state_dict(hp, 0), strict=False)
    m = m.to("cuda").eval()
    m.load_posterior(synth.synthetic_posterior_state_dict(hp, 0))
    for name, sh in SHAPES.items():
        if a.shape and name != a.shape:
            continue
        xl, yl = sh["x"], sh["y"]
        B, T, Ty = len(xl), max(xl), max(yl)
        batch = synth.synthetic_batch(xl, languages=[i % 3 for i in range(B)], sids=list(range(B)))
        dev = lambda k: batch[k].cuda()
        enc = m.encode_durations(dev("x"), dev("x_lengths"), dev("sid"), dev("tone"), dev("language"), dev("bert"), dev("ja_bert"),
                                 dev("en_bert"), models.draw_noise_w(B, T, None), sdp_ratio=0.0, lean=True)
        g = torch.Generator().manual_seed(1)
        y = torch.rand(B, hp.spec_channels, Ty, generator=g).cuda()
        yl_d, xl_d = torch.tensor(yl).cuda(), torch.tensor(xl).cuda()
        whole = lambda: m.align(dev("x"), xl_d, dev("sid"), dev("tone"), dev("language"), dev("bert"), dev("ja_bert"), dev("en_bert"), y, yl_d)
        if a.trace_calls:
            torch.cuda.synchronize()
            for _ in range(a.trace_calls):
                whole()
            torch.cuda.synchronize()
            print(json.dumps(dict(shape=name, traced_align_calls=a.trace_calls)), flush=True)
            continue
        z = m.posterior_encode(y, yl_d, g=enc["g"])["z"]
        z_p = m.stage_flow_forward(z, yl_d, enc["g"])
        nc = align.neg_cent(z_p, enc["m_p"], enc["logs_p"], xl_d, yl_d)
        rows = [
            ("phase_a", lambda: m.encode_durations(dev("x"), dev("x_lengths"), dev("sid"), dev("tone"), dev("language"), dev("bert"), dev("ja_bert"),
                                                   dev("en_bert"), models.draw_noise_w(B, T, None), sdp_ratio=0.0, lean=True), None),
            ("enc_q", lambda: m.posterior_encode(y, yl_d, g=enc["g"]), 37),
            ("flow_forward", lambda: m.stage_flow_forward(z, yl_d, enc["g"]), None),
            ("neg_cent", lambda: align.neg_cent(z_p, enc["m_p"], enc["logs_p"], xl_d, yl_d), 1),
            ("maximum_path", lambda: align.maximum_path(nc, xl_d, yl_d), 1),
            ("maximum_path+attn", lambda: align.maximum_path(nc, xl_d, yl_d, want_attn=True), 1),
            ("align_latent", lambda: m.align_latent(enc, z_p, yl_d, x_lengths=xl_d), 2),
            ("align", whole, None),
        ]
        for what, fn, launches in rows:
            calls = max(5, a.calls // (8 if B > 1 else 1))
            med, runs = _median_us(fn, calls)
            rec = dict(shape=name, B=B, T=T, Ty=Ty, what=what, median_us=med, runs_us=runs, launches=launches)
            if what.startswith("maximum_path"):
                rec["us_per_row"] = round(med / Ty, 3)
            print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
