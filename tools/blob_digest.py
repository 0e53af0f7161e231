#!/usr/bin/env python3
"""sha256 of the packed weight blobs (``pack_host_blob``, ``pack_posterior_host_blob`` and ``pack_sdp_forward_host_blob``) of a fixed set of
models with seeded synthetic weights.  Packing is CPU-only, so this runs without a GPU.  A change that is meant to leave the blob alone (a
refactor of the packer, a new writer for an old format) must print the same listing before and after:

    python tools/blob_digest.py > after.txt        # and the same in a checkout of the parent commit; diff the two

    python tools/blob_digest.py --time 3           # also: seconds per pack_host_blob() of the full-size model, 3 runs
"""
import argparse
import hashlib
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bert_vits2_amd import hparams as H, models, synth  # noqa: E402
from oracle import cases  # noqa: E402

SEED = 20241019
MODELS = [
    ("v23_full", {}),                                              # the benchmark's model (BASELINE config 2): transformer flow, 4 couplings
    ("v23_wn_flow", dict(use_transformer_flow=False)),
    ("v23_resblock2", cases.CASES["rb2_b2_t14"]["hp"]),
    ("v23_ref_enc", dict(n_speakers=0)),                           # no speaker table: the ReferenceEncoder's tensors are in the blob
    ("hp01_tf3_c16", cases.ENVELOPE["hp01_tf3_h128x4"]["hp"]),     # odd coupling count; last stage C = 16: both whole-ResBlock streams
    ("hp09_wn5_k11", cases.ENVELOPE["hp09_wn5_h256x2"]["hp"]),     # odd WN coupling count, k = 11 at C = 16
    ("narrow", cases.CASES["narrow_b2_t18"]["hp"]),
]


def sha(t):
    return hashlib.sha256(t.numpy().tobytes()).hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--time", type=int, default=0, metavar="N", help="time N runs of pack_host_blob() of the full-size model")
    args = ap.parse_args()
    for name, ov in MODELS:
        hp = H.default_v23(**ov)
        m = models.from_hparams(hp)
        m.load_state_dict(synth.synthetic_state_dict(hp, SEED), strict=False)
        blob = m.pack_host_blob()
        print(f"{name:14s} inference {blob.numel():>11d} bytes {sha(blob)}")
        post = m.pack_posterior_host_blob(synth.synthetic_posterior_state_dict(hp, SEED))
        print(f"{name:14s} posterior {post.numel():>11d} bytes {sha(post)}")
        try:
            sdpf = m.pack_sdp_forward_host_blob(synth.synthetic_sdp_forward_state_dict(hp, SEED))
            print(f"{name:14s} sdp_forward {sdpf.numel():>9d} bytes {sha(sdpf)}")
        except RuntimeError as e:                                  # hidden_channels the whole-layer DDSConv kernel does not support
            print(f"{name:14s} sdp_forward refused: {str(e).split(': ', 1)[-1]}")
        if name == "v23_full":
            for _ in range(args.time):
                t0 = time.perf_counter()
                m.pack_host_blob()
                print(f"{name:14s} pack_host_blob {time.perf_counter() - t0:.3f} s")


if __name__ == "__main__":
    main()
