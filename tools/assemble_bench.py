#!/usr/bin/env python3
"""Timings for documents joined on the device (docs/MEASUREMENTS.md, "Documents").  GPU only.

    python tools/assemble_bench.py [--calls 20] [--paragraphs 4] [--sentences 10] [--symbols 154]

One document of ``paragraphs x sentences`` sentences of ``symbols`` symbols each on the full-size model with bench.py's seeded checkpoint
(2.5 frames per symbol: 154 symbols are 4.46 s), every utterance seeded:

  (a) the way without this feature: ``serving.synthesize(as_pcm16=True)`` and the join in numpy (int16 pieces and int16 zero pauses
      concatenated on the host — cheaper than the reference's fp64 tail, so the bar is not lowered);
  (b) ``serving.synthesize_documents``.

Both are timed with the host clock from the call to the host array, alternating, after warm-up; median and all runs.  The bits of (a) and
(b) are compared first.  Then ``bv2_assemble`` alone on the same shapes (40 pieces in two tensors, 16-bit output), HIP events around
repeated calls of the C entry point: the layout launch alone (``max_capacity = 0`` launches nothing else), layout + write (level NONE) and
layout + peaks + write (PIECE_PEAK); the write launch is the difference of the first two, its GB/s counts 4 bytes read and 2 written per
sample of the document's total.  One JSON line each."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bert_vits2_amd import audio, hparams as H, lib as L, models, serving, synth  # noqa: E402


def utterances(n, T):
    out = []
    for i in range(n):
        b = synth.synthetic_batch([T], languages=[i % 3], sids=[i * 7 % 50], first_index=i)
        out.append(serving.Utterance(b["x"][0], b["tone"][0], b["language"][0], b["bert"][0], b["ja_bert"][0], b["en_bert"][0],
                                     int(b["sid"][0]), seed=100 + i))
    return out


def host_join(pieces, paragraphs, sentences, rate):
    sent, extra = audio.pause_samples(rate, 0.2), audio.paragraph_pause_samples(rate, 1.0, 0.2)
    out = []
    for p in range(paragraphs):
        for s in range(sentences):
            out += [pieces[p * sentences + s], np.zeros(sent, np.int16)]
        out.append(np.zeros(extra, np.int16))
    return np.concatenate(out)


def launches_alone(rows, S, calls, dev_name):
    lib = L.load()
    split = min(32, rows)
    src = [torch.rand(split, S, device="cuda") - 0.5] + ([torch.rand(rows - split, S, device="cuda") - 0.5] if rows > split else [])
    lens = [torch.full((t.shape[0],), S // 512, dtype=torch.int64, device="cuda") for t in src]
    segments = []
    for i in range(rows):
        segments += [audio.Piece(i // split, i % split, 0, 0), audio.Silence(8820, 0)]
    table, n_groups, n_docs = audio._segment_table(src, [(t, 512) for t in lens], segments)
    res = dict(what="bv2_assemble alone", pieces=rows, S=S, device=dev_name, calls_per_run=calls)
    total = None
    for name, level, grid in (("layout", "none", False), ("layout_write", "none", True), ("layout_peaks_write", "piece", True)):
        capacity, _ = audio.assemble_plan(table, n_groups, n_docs, level, True)
        cfg = audio.assemble_config(level, True, max(capacity) if grid else 0)
        n = len(table)
        tb = C.sizeof(L.AssembleSegment) * n
        host = np.empty(tb + 16, np.uint8)
        host[:tb] = np.frombuffer(table, np.uint8)
        dst = torch.empty(capacity[0], dtype=torch.int16, device="cuda")
        host[tb:].view(np.int64)[:] = [dst.data_ptr(), capacity[0]]
        blob = torch.from_numpy(host).cuda()
        ws = torch.empty(lib.bv2_assemble_workspace_bytes(C.byref(cfg), n, n_groups, n_docs), dtype=torch.uint8, device="cuda")
        offsets, totals = torch.empty(n, dtype=torch.int64, device="cuda"), torch.empty(1, dtype=torch.int64, device="cuda")
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

        def call():
            rc = lib.bv2_assemble(stream, C.byref(cfg), C.c_void_p(blob.data_ptr()), n, n_groups, n_docs, None, C.c_void_p(blob.data_ptr() + tb),
                                  C.c_void_p(blob.data_ptr() + tb + 8), C.c_void_p(offsets.data_ptr()), C.c_void_p(totals.data_ptr()),
                                  C.c_void_p(ws.data_ptr()), ws.numel())
            assert rc == 0, lib.bv2_last_error(None).decode()

        for _ in range(20):
            call()
        torch.cuda.synchronize()
        runs = []
        for _ in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                call()
            e1.record()
            e1.synchronize()
            runs.append(round(1e3 * e0.elapsed_time(e1) / calls, 2))
        res["us_" + name], res["runs_" + name] = statistics.median(runs), runs
        total = int(totals.cpu()[0])
    res["samples"] = total
    res["us_write"] = round(res["us_layout_write"] - res["us_layout"], 2)
    res["us_peaks"] = round(res["us_layout_peaks_write"] - res["us_layout_write"], 2)
    res["write_GBps"] = round(6.0 * total / (res["us_write"] * 1e-6) / 1e9, 1) if res["us_write"] > 0 else None
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--paragraphs", type=int, default=4)
    ap.add_argument("--sentences", type=int, default=10)
    ap.add_argument("--symbols", type=int, default=154)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/assemble_bench.py needs a GPU")
    dev_name = torch.cuda.get_device_name(0)
    hp = H.default_v23()
    m = models.from_hparams(hp)
    m.load_state_dict(synth.synthetic_state_dict(hp, seed=0, pin_durations=2.5), strict=False)
    m = m.to("cuda").eval()
    rate = hp.sampling_rate
    P, S = args.paragraphs, args.sentences
    utts = utterances(P * S, args.symbols)
    docs = [[[utts[p * S + s] for s in range(S)] for p in range(P)]]

    def way_a():
        return host_join(serving.synthesize(m, utts, as_pcm16=True), P, S, rate)

    def way_b():
        return serving.synthesize_documents(m, docs)[0]

    a, b = way_a(), way_b()
    same = bool(a.shape == b.shape and np.array_equal(a, b))
    for _ in range(3):
        way_a(), way_b()
    runs = {"a": [], "b": []}
    for _ in range(args.calls):
        for key, fn in (("a", way_a), ("b", way_b)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            runs[key].append(round(1e3 * (time.perf_counter() - t0), 3))
    print(json.dumps(dict(what="one document, call to host array", paragraphs=P, sentences=S, symbols=args.symbols, samples=int(a.size),
                          seconds=round(a.size / rate, 2), same_bits=same, device=dev_name,
                          ms_a_synthesize_plus_numpy_join=statistics.median(runs["a"]), ms_b_synthesize_documents=statistics.median(runs["b"]),
                          runs_a=runs["a"], runs_b=runs["b"])), flush=True)
    launches_alone(P * S, 196608, 200, dev_name)


if __name__ == "__main__":
    main()
