"""Generate ``tests/golden/item_controls_*.npz``: the REAL reference run with per-utterance synthesis controls — build-container only.

    python tools/gen_item_controls_golden.py        # from the repo root, needs the reference checkout (oracle.ref_import)

The reference's ``SynthesizerTrn.infer`` takes ``sdp_ratio``, ``noise_scale``, ``noise_scale_w`` and ``length_scale`` as values torch
broadcasts, so one value per utterance can be handed over as a ``[B,1,1]`` tensor.  Each case below runs the reference that way on a
ragged batch of the ``narrow_b2_t18`` model (oracle/cases.py), with the seeded weights, utterances and injected noise of the other
fixtures, and stores what it returned in the format of ``oracle/gen_golden.py``.  Across the two cases every control takes four
distinct values.

Two facts are checked on the way and recorded in the fixture's metadata:
  * the reference's tensor form computes ``1 - sdp_ratio`` in fp32, the library's per-utterance path as
    ``(float)(1.0 - (double)r)`` (the rounding of its scalar path): the two agree for every ratio used here;
  * per utterance, the batched run's durations equal a batch-1 reference run with that utterance's values as Python scalars.
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bert_vits2_amd import hparams as H, synth  # noqa: E402
from oracle import cases, ref_import  # noqa: E402

MODEL_CASE = "narrow_b2_t18"
CONTROL_ORDER = ("noise_scale_w", "sdp_ratio", "length_scale", "noise_scale")     # the member order of bv2_item_controls
ITEM_CASES = {
    "item_controls_narrow_b3": dict(lengths=[18, 11, 7], languages=[0, 1, 2], sids=[2, 640, 77],
                                    controls=dict(sdp_ratio=[0.2, 0.8, 0.5], noise_scale=[0.3, 0.9, 0.6],
                                                  noise_scale_w=[0.5, 1.1, 0.8], length_scale=[0.8, 1.3, 1.0])),
    "item_controls_narrow_b2": dict(lengths=[15, 9], languages=[2, 0], sids=[5, 300],
                                    controls=dict(sdp_ratio=[1.0, 0.2], noise_scale=[0.667, 0.3],
                                                  noise_scale_w=[0.9, 0.5], length_scale=[1.15, 0.8])),
}
KEYS = ["o", "logw", "logw_sdp", "logw_dp", "w_ceil", "y_mask", "attn"]


def build_inputs(c):
    """(hp, weight seed, batch, noise_w, noise_z) of an item-controls case — what the tests rebuild from the fixture's metadata."""
    base = cases.CASES[MODEL_CASE]
    hp = H.default_v23(**base["hp"])
    batch = synth.synthetic_batch(c["lengths"], c["languages"], c["sids"])
    B, T = batch["x"].shape
    noise_w, noise_z = synth.synthetic_noise(B, T, cases.T_Y_CAP, hp.inter_channels)
    return hp, base["seed"], batch, noise_w, noise_z


def item(batch, noise_w, noise_z, b, n):
    """Utterance b of a padded batch on its own (its n symbols), as a batch-1 caller hands it over."""
    one = {k: v[b:b + 1] for k, v in batch.items()}
    for k in ("x", "tone", "language"):
        one[k] = one[k][:, :n]
    for k in ("bert", "ja_bert", "en_bert"):
        one[k] = one[k][:, :, :n]
    return one, noise_w[b:b + 1, :, :n], noise_z[b:b + 1]


def main():
    torch.set_num_threads(1)
    torch.use_deterministic_algorithms(True)
    out_dir = os.path.join(ROOT, "tests", "golden")
    nets = {}
    for name, c in ITEM_CASES.items():
        hp, seed, batch, noise_w, noise_z = build_inputs(c)
        if seed not in nets:
            sd = synth.synthetic_state_dict(hp, seed)
            nets[seed] = (sd, ref_import.build_reference_net(hp, sd))
        sd, net = nets[seed]
        B = len(c["lengths"])
        ctl = {k: torch.tensor(c["controls"][k], dtype=torch.float32).view(B, 1, 1) for k in CONTROL_ORDER}
        for r in ctl["sdp_ratio"].flatten():
            assert float(1 - r) == float(np.float32(1.0 - float(r))), "fp32 1 - r differs from the double-rounded form"
        ref = ref_import.reference_infer(net, batch, noise_w, noise_z, **ctl)
        arrays = {k: ref[k].detach().float().numpy() for k in KEYS}
        y_lengths = ref["y_mask"].sum([1, 2]).long()
        arrays["y_lengths"] = y_lengths.numpy()
        arrays["controls"] = np.stack([ctl[k].flatten().numpy() for k in CONTROL_ORDER])      # [4, B]
        for b, n in enumerate(c["lengths"]):
            one, nw, nz = item(batch, noise_w, noise_z, b, n)
            kw = {k: float(c["controls"][k][b]) for k in CONTROL_ORDER}
            r1 = ref_import.reference_infer(net, one, nw, nz, **kw)
            assert torch.equal(r1["w_ceil"][0, 0, :n], ref["w_ceil"][b, 0, :n]), (name, b)
            assert int(r1["y_mask"].sum()) == int(y_lengths[b]), (name, b)
        meta = dict(case=name, model_case=MODEL_CASE, lengths=c["lengths"], languages=c["languages"], sids=c["sids"],
                    controls=c["controls"], control_order=list(CONTROL_ORDER), torch=torch.__version__,
                    checksums=cases.weight_checksums(sd), o_rms=float(ref["o"].pow(2).mean().sqrt()), T_y=int(ref["y_mask"].shape[2]),
                    one_minus_ratio="fp32 1 - r equals (float)(1.0 - (double)r) for every sdp_ratio of this case",
                    batch1_durations="every utterance's w_ceil / y_length equal a batch-1 reference run with its values as scalars")
        path = os.path.join(out_dir, name + ".npz")
        np.savez_compressed(path, meta=json.dumps(meta), **arrays)
        print(name, os.path.getsize(path), "bytes", {k: v.shape for k, v in arrays.items()}, "y_lengths", arrays["y_lengths"].tolist())


if __name__ == "__main__":
    main()
