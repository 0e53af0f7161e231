#!/usr/bin/env python3
"""Latency of streamed synthesis against the whole decode (docs/MEASUREMENTS.md, "Streamed synthesis").  GPU only.

    python tools/stream_latency.py [--chunks 64 128] [--reps 12]

Two shapes: config 2 (B = 1 x 128 symbols, fp32) and config 5's shape (B = 8 x 512 symbols, bf16 Generator + fp16 flow), durations pinned to 3
frames per symbol (T_y = 384 / 1536).  Per shape and chunk size, in one process, alternating:
  whole     infer(want_attn=False, exact_lengths=True), the waveform copied to pinned host memory, the host waits for the copy
  streamed  infer_stream(same), every chunk copied to one of two pinned buffers, chunk n + 1 enqueued before the host waits on chunk n
            (what serving.synthesize_stream does); the clock is read when the FIRST chunk is on the host and when the LAST one is
Times are host wall-clock from the call to the moment the bytes are on the host (medians over --reps); the workspace bytes of both plans
come from bv2_workspace_bytes / bv2_stream_workspace_bytes.  One JSON line per measurement."""
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

KW = dict(noise_scale=0.6, noise_scale_w=0.9, sdp_ratio=0.0, length_scale=1.0, want_attn=False, exact_lengths=True)


def whole(m, a, host):
    t0 = time.perf_counter()
    o = m.infer(*a, **KW)[0]
    host.copy_(o[:, 0], non_blocking=True)
    ev = torch.cuda.Event()
    ev.record()
    ev.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def streamed(m, a, hosts, chunk, first):
    t0 = time.perf_counter()
    st = m.infer_stream(*a, chunk_frames=chunk, first_chunk_frames=first, **KW)
    waiting, t_first = None, None
    for k, (_, audio) in enumerate(st):
        hosts[k & 1][:, :audio.shape[1]].copy_(audio, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        if waiting is not None:
            waiting.synchronize()
            t_first = t_first or time.perf_counter()
        waiting = ev
    waiting.synchronize()
    t_end = time.perf_counter()
    return 1e3 * ((t_first or t_end) - t0), 1e3 * (t_end - t0), len(st)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", type=int, nargs="+", default=[64, 128])
    ap.add_argument("--first", type=int, default=0, help="first_chunk_frames (0 = the chunk size)")
    ap.add_argument("--reps", type=int, default=12)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("tools/stream_latency.py needs a GPU")
    torch.manual_seed(0)
    hp = H.default_v23()
    m = models.from_hparams(hp)
    m.load_state_dict(synth.synthetic_state_dict(hp, 0, pin_durations=2.5), strict=False)
    m = m.to("cuda").eval()
    U = hp.total_upsample
    for name, B, T, reduced in (("config2", 1, 128, False), ("config5_shape", 8, 512, True)):
        if reduced:
            m.set_generator_dtype(torch.bfloat16)
            m.set_flow_dtype(torch.float16)
        batch = synth.synthetic_batch([T] * B, [i % 3 for i in range(B)], [(7 * i) % hp.n_speakers for i in range(B)])
        a = [batch[k].cuda() for k in ("x", "x_lengths", "sid", "tone", "language", "bert", "ja_bert", "en_bert")]
        Ty = m.infer(*a, **KW)[0].shape[2] // U            # 3 frames per symbol with the pinned durations
        host = torch.empty(B, Ty * U, dtype=torch.float32, pin_memory=True)
        for chunk in args.chunks:
            first = args.first or None
            hosts = [torch.empty(B, max(chunk, first or 0) * U, dtype=torch.float32, pin_memory=True) for _ in range(2)]
            for _ in range(3):
                whole(m, a, host)
                streamed(m, a, hosts, chunk, first)
            w, f, t, n = [], [], [], 0
            for _ in range(args.reps):
                w.append(whole(m, a, host))
                tf, tt, n = streamed(m, a, hosts, chunk, first)
                f.append(tf)
                t.append(tt)
            med = statistics.median
            ws_whole = m._lib.bv2_workspace_bytes(m._handle, B, T, Ty)
            ws_stream = m._lib.bv2_stream_workspace_bytes(m._handle, B, T, Ty, max(chunk, first or 0))
            print(json.dumps(dict(what=f"{name}: streamed vs whole", B=B, T=T, Ty=Ty, generator="bf16" if reduced else "fp32",
                                  flow="fp16" if reduced else "fp32", chunk_frames=chunk, first_chunk_frames=first or chunk, chunks=n,
                                  halo=H.generator_halo(hp), ms_whole_on_host=round(med(w), 3), ms_first_chunk_on_host=round(med(f), 3),
                                  ms_last_chunk_on_host=round(med(t), 3), first_over_whole=round(med(f) / med(w), 3),
                                  total_over_whole=round(med(t) / med(w), 3), workspace_bytes_whole=int(ws_whole),
                                  workspace_bytes_streamed=int(ws_stream), reps=args.reps, device=torch.cuda.get_device_name(0))), flush=True)


if __name__ == "__main__":
    main()
