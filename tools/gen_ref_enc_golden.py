"""Generate ``tests/golden/ref_enc_*.npz``: the REAL reference's ReferenceEncoder path (``n_speakers = 0``) — build-container only.

    python tools/gen_ref_enc_golden.py        # from the repo root, needs the reference checkout (oracle.ref_import)

Two fixtures, both small (the spectrograms are rebuilt by the tests from the metadata with ``synth.synthetic_reference_spec``):

``ref_enc_g.npz``          ``g`` of the reference's ``ReferenceEncoder`` module run ALONE at batch 1, for every spectrogram width of the
                           accepted envelope (1025 and 513: odd chains of the ``(n - 1) // 2 + 1`` arithmetic, 80: an even one) and
                           L in {61, 96, 400, 7} (7 collapses to one GRU step).  Per case the module is also evaluated in fp64:
                           ``g64`` is that result, ``ref_err = max|g_fp32 - g_fp64|`` the reference's own fp32 error and ``rms`` the
                           scale of ``g64`` — the GPU test's bar is built from ``ref_err`` of the case, not from a constant.
``ref_enc_narrow_b2.npz``  the ``narrow_b2_t18`` model (oracle/cases.py) built with ``n_speakers = 0`` and ``spec_channels = 1025``, run end to
                           end by the reference's ``infer(..., y=y)``: text lengths [18, 11], both references L = 61 (equal and odd, so the
                           reference's unmasked batch is legitimate).  The keys of the item-controls fixtures plus ``z`` and ``g`` (taken by
                           a forward hook on ``ref_enc``).

Durations must not sit on a knife edge: the end-to-end case is run a second time with ``g`` replaced by the fp64 module's output
rounded to fp32, and ``w_ceil`` / ``y_lengths`` must come out identical.  That is a condition on the INPUTS (weights seed, lengths,
spectrograms), checked here on the CPU; it is what entitles the GPU test to demand exact durations.  The choice that satisfies it is
recorded in the fixture's metadata (``knife_edge``).
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
SPECS = (1025, 513, 80)
LENGTHS = (61, 96, 400, 7)
E2E = dict(name="ref_enc_narrow_b2", spec_channels=1025, ref_lengths=[61, 61], ref_index=[0, 1])
KEYS = ["o", "logw", "logw_sdp", "logw_dp", "w_ceil", "y_mask", "attn", "z"]


def model_hparams(spec_channels):
    """The narrow_b2_t18 model without a speaker table."""
    base = cases.CASES[MODEL_CASE]
    return H.default_v23(**dict(base["hp"], n_speakers=0, spec_channels=spec_channels)), base


def g_case_name(spec, L):
    return f"s{spec}_l{L}"


def ref_enc_module(hp, sd, dtype=torch.float32):
    """The reference's ReferenceEncoder alone, loaded with the ``ref_enc.*`` tensors of ``sd``."""
    models = ref_import.reference_models()
    mod = models.ReferenceEncoder(hp.spec_channels, hp.gin_channels).eval()
    missing, unexpected = mod.load_state_dict({k[len("ref_enc."):]: v for k, v in sd.items() if k.startswith("ref_enc.")}, strict=True)
    assert not missing and not unexpected
    return mod.to(dtype)


@torch.no_grad()
def run_module(mod, y):
    """``ref_enc(y.transpose(1, 2))`` as reference models.py:1048 calls it; y [B, spec, L]."""
    return mod(y.transpose(1, 2))


def main():
    torch.set_num_threads(1)
    torch.use_deterministic_algorithms(True)
    out_dir = os.path.join(ROOT, "tests", "golden")

    # ---- g of the module alone, batch 1
    arrays, gmeta = {}, {}
    for spec in SPECS:
        hp, base = model_hparams(spec)
        sd = synth.synthetic_state_dict(hp, base["seed"])
        m32, m64 = ref_enc_module(hp, sd), ref_enc_module(hp, sd, torch.float64)
        for L in LENGTHS:
            y = synth.synthetic_reference_spec(spec, L, 0)[None]
            g32 = run_module(m32, y)[0]
            g64 = run_module(m64, y.double())[0]
            name = g_case_name(spec, L)
            arrays[name + "_g"] = g32.numpy()
            arrays[name + "_g64"] = g64.numpy()
            ref_err = float((g32.double() - g64).abs().max())
            rms = float(g64.pow(2).mean().sqrt())
            gmeta[name] = dict(spec_channels=spec, L=L, index=0, ref_err=ref_err, rms=rms)
            print(f"{name}: ref_err {ref_err:.3e}  rms {rms:.4f}  ref_err/rms {ref_err / rms:.2e}  |g|max {float(g64.abs().max()):.3f}")
    meta = dict(model_case=MODEL_CASE, seed=cases.CASES[MODEL_CASE]["seed"], gin_channels=model_hparams(1025)[0].gin_channels,
                cases=gmeta, torch=torch.__version__,
                note="g = reference ReferenceEncoder alone at batch 1 (fp32), g64 = the same module in fp64")
    path = os.path.join(out_dir, "ref_enc_g.npz")
    np.savez_compressed(path, meta=json.dumps(meta), **arrays)
    print("ref_enc_g", os.path.getsize(path), "bytes")

    # ---- end to end
    hp, base = model_hparams(E2E["spec_channels"])
    seed = base["seed"]
    sd = synth.synthetic_state_dict(hp, seed)
    net = ref_import.build_reference_net(hp, sd)
    batch = synth.synthetic_batch(base["lengths"], base["languages"], base["sids"])
    B, T = batch["x"].shape
    noise_w, noise_z = synth.synthetic_noise(B, T, cases.T_Y_CAP, hp.inter_channels)
    kw = dict(base["kw"])
    y = torch.stack([synth.synthetic_reference_spec(hp.spec_channels, L, i) for L, i in zip(E2E["ref_lengths"], E2E["ref_index"])])
    tap = {}
    hk = net.ref_enc.register_forward_hook(lambda mod, inp, out: tap.__setitem__("g", out))
    ref = ref_import.reference_infer(net, batch, noise_w, noise_z, y=y, **kw)
    hk.remove()
    g = tap["g"].detach()
    y_lengths = ref["y_mask"].sum([1, 2]).long()
    # the knife-edge condition: the same run on the fp64 module's g (rounded to fp32) gives the same durations
    g64 = run_module(ref_enc_module(hp, sd, torch.float64), y.double()).float()
    hk = net.ref_enc.register_forward_hook(lambda mod, inp, out: g64)       # a hook's return value replaces the module's output
    ref2 = ref_import.reference_infer(net, batch, noise_w, noise_z, y=y, **kw)
    hk.remove()
    assert torch.equal(ref2["w_ceil"], ref["w_ceil"]), "durations sit on a knife edge: change the seed / lengths / spectrograms"
    assert torch.equal(ref2["y_mask"].sum([1, 2]).long(), y_lengths)
    wave_shift = float((ref2["o"] - ref["o"]).pow(2).mean().sqrt())
    arr = {k: ref[k].detach().float().numpy() for k in KEYS}
    arr["y_lengths"] = y_lengths.numpy()
    arr["g"] = g.numpy()
    meta = dict(case=E2E["name"], model_case=MODEL_CASE, seed=seed, spec_channels=hp.spec_channels, ref_lengths=E2E["ref_lengths"],
                ref_index=E2E["ref_index"], lengths=base["lengths"], languages=base["languages"], sids=base["sids"], kw=kw,
                torch=torch.__version__, checksums=cases.weight_checksums(sd), o_rms=float(ref["o"].pow(2).mean().sqrt()),
                T_y=int(ref["y_mask"].shape[2]),
                g_ref_err=float((g.double() - run_module(ref_enc_module(hp, sd, torch.float64), y.double())).abs().max()),
                knife_edge=f"weights seed {seed}, references index {E2E['ref_index']} at L = {E2E['ref_lengths']}: w_ceil and y_lengths are identical "
                           f"with g from the fp64 module rounded to fp32 (the wave moves by {wave_shift:.2e} rms)")
    path = os.path.join(out_dir, E2E["name"] + ".npz")
    np.savez_compressed(path, meta=json.dumps(meta), **arr)
    print(E2E["name"], os.path.getsize(path), "bytes", {k: v.shape for k, v in arr.items()}, "y_lengths", arr["y_lengths"].tolist(),
          "o rms", meta["o_rms"], "| wave shift with fp64 g", wave_shift)


if __name__ == "__main__":
    main()
