"""Generate ``tests/golden/score_*.npz``: the REAL reference's duration likelihood and KL term — build-container only.

    python tools/gen_score_golden.py      # from the repo root, needs the reference checkout (oracle.ref_import)

Duration likelihood (``score_<case>.npz``).  The reference net is built from ``synth.synthetic_state_dict`` +
``synthetic_posterior_state_dict`` + ``synthetic_sdp_forward_state_dict`` and its own ``net.sdp(x, x_mask, w, g=g)`` (models.py:197-244) is
called on stored inputs: ``x`` (an encoder-output-like tensor), ``g``, the durations ``w`` and ``noise_e``, which is handed to the one
``torch.randn`` of models.py:215.  Every case runs in fp32 and once more with the module in ``.double()``; ``ref_err_nll`` =
max |fp32 - fp64| of the reference's own result.  The per-position decomposition comes from the restatement (tests/score_oracle.py) in
fp64, with ``ref_err_nll_sym`` = max |fp32 - fp64| of the restatement per element (the reference returns one number per item).

The single-length cases hold FOUR utterances of that length (own ``x``, ``g``, ``w``, ``noise_e``): ``ref_err_nll`` is a maximum, and the
maximum over one number is whatever rounding luck that number had — a first draft with one utterance per case gave T = 17 a reference
error of 5.8e-6 on a value of 374, a fifth of that value's fp32 spacing, which no fp32 computation can be asked to repeat.

KL (``score_kl_<case>.npz``).  On the ``z_p / logs_q / m_p / logs_p`` and durations of ``posterior_<case>.npz``, the prior gathered along
the path, the reference's ``losses.kl_loss`` gives the fp32 value per item (it casts to float, so its fp64 twin is its own expression
evaluated on doubles here); ``ref_err_kl`` = max |fp32 - fp64|.
"""
from __future__ import annotations

import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bert_vits2_amd import hparams as H, synth  # noqa: E402
from oracle import cases, ref_import  # noqa: E402
from tests import score_oracle as SO  # noqa: E402
from tests.helpers import load_golden  # noqa: E402

NARROW = cases.CASES["narrow_b2_t18"]["hp"]
# name: hp overrides, symbols per item, (item, symbol) pairs whose duration is 0
CASES = {
    "t1": dict(hp={}, lengths=[1] * 4),
    "t3": dict(hp={}, lengths=[3] * 4),                    # below the dilated depthwise reach
    "t17": dict(hp={}, lengths=[17] * 4),                  # across the 16-step tile of the DDS kernel
    "t18": dict(hp={}, lengths=[18] * 4),
    "b2_ragged": dict(hp={}, lengths=[18, 11]),
    "zero_dur": dict(hp={}, lengths=[18] * 4, zero=[(0, 5), (0, 12), (2, 0), (3, 17)]),   # the clamp_min(1e-5) branch of Log
    "narrow_b2_t18": dict(hp=NARROW, lengths=[18, 11]),    # hidden 128
}
KL_CASES = ["narrow_b2_t18", "mix_b2_ragged", "wn_b1_t16"]
SEED, INPUT_SEED = 0, 8642


def inputs(hp, lengths, zero=()):
    g = torch.Generator().manual_seed(INPUT_SEED + 17 * len(lengths) + max(lengths))
    B, T = len(lengths), max(lengths)
    mask = (torch.arange(T)[None, :] < torch.tensor(lengths)[:, None]).float()[:, None]
    x = torch.randn(B, hp.hidden_channels, T, generator=g) * mask
    gv = torch.randn(B, hp.gin_channels, 1, generator=g)
    w = torch.randint(1, 7, (B, 1, T), generator=g).float() * mask
    for b, t in zero:
        w[b, 0, t] = 0.0
    noise_e = torch.randn(B, 2, T, generator=g)
    return x, mask, w, gv, noise_e


@torch.no_grad()
def reference_nll(net, x, mask, w, g, noise_e, dtype):
    real, draws = torch.randn, []

    def fake(*size, **kw):
        shape = tuple(size[0]) if len(size) == 1 and isinstance(size[0], (tuple, list, torch.Size)) else tuple(size)
        assert shape == tuple(noise_e.shape), (shape, noise_e.shape)
        draws.append(1)
        return noise_e.clone()

    torch.randn = fake
    try:
        out = net.sdp(x.to(dtype), mask.to(dtype), w.to(dtype), g=g.to(dtype))
    finally:
        torch.randn = real
    assert len(draws) == 1 and out.dtype == dtype
    return out


def reference_kl_loss():
    for name in ("torchaudio", "transformers"):          # losses.py imports them for its WavLM loss only
        if name not in sys.modules:
            try:
                __import__(name)
            except Exception:
                m = types.ModuleType(name)
                m.AutoModel = None
                sys.modules[name] = m
    ref_import.reference_models()
    import losses
    return losses.kl_loss


def main():
    torch.set_num_threads(1)
    torch.use_deterministic_algorithms(True)
    out_dir = os.path.join(ROOT, "tests", "golden")
    nets = {}
    for name, cs in CASES.items():
        hp = H.default_v23(**cs["hp"])
        key = repr(sorted(cs["hp"].items()))
        if key not in nets:
            sd = synth.synthetic_state_dict(hp, SEED)
            sd.update(synth.synthetic_posterior_state_dict(hp, SEED))
            sd.update(synth.synthetic_sdp_forward_state_dict(hp, SEED))
            nets[key] = (sd, ref_import.build_reference_net(hp, sd), ref_import.build_reference_net(hp, sd).double())
        sd, net32, net64 = nets[key]
        x, mask, w, g, noise_e = inputs(hp, cs["lengths"], cs.get("zero", ()))
        nll32 = reference_nll(net32, x, mask, w, g, noise_e, torch.float32)
        nll64 = reference_nll(net64, x, mask, w, g, noise_e, torch.float64)
        sd32 = {k: v for k, v in sd.items() if k.startswith("sdp.")}
        sd64 = {k: v.double() for k, v in sd32.items()}
        o32, sym32 = SO.sdp_forward(sd32, x, mask, w, g, noise_e)
        o64, sym64 = SO.sdp_forward(sd64, x.double(), mask.double(), w.double(), g.double(), noise_e.double())
        meta = dict(case=name, seed=SEED, hp=cs["hp"], lengths=cs["lengths"], zero=cs.get("zero", []), torch=torch.__version__,
                    checksums=cases.weight_checksums(sd), ref_err_nll=float((nll32.double() - nll64).abs().max()),
                    ref_err_nll_sym=float((sym32.double() - sym64).abs().max()),
                    oracle_vs_reference=float(((o64 - nll64).abs() / nll64.abs()).max()),
                    note="net.sdp(x, x_mask, w, g=g) of the reference in fp32 / fp64 (nll64); nll_sym64: the restatement's decomposition")
        path = os.path.join(out_dir, "score_" + name + ".npz")
        np.savez_compressed(path, meta=json.dumps(meta), x=x.numpy(), x_mask=mask.numpy(), w=w.numpy(), g=g.numpy(), noise_e=noise_e.numpy(),
                            nll64=nll64.numpy(), nll_sym64=sym64.numpy())
        print(f"{name}: {os.path.getsize(path)} bytes; nll64 {nll64.tolist()} ref_err_nll {meta['ref_err_nll']:.3e} "
              f"ref_err_nll_sym {meta['ref_err_nll_sym']:.3e} restatement vs reference (rel) {meta['oracle_vs_reference']:.2e}")

    kl_loss = reference_kl_loss()
    for name in KL_CASES:
        _meta, G = load_golden("posterior_" + name)
        z_p, logs_q, m_p, logs_p = G["z_p"], G["logs_q64"].float(), G["m_p"], G["logs_p"]
        dur, xl, yl = G["durations"], G["x_lengths"].tolist(), G["y_lengths"].tolist()
        B, C, Ty = z_p.shape
        kl32, kl64 = torch.zeros(B), torch.zeros(B, dtype=torch.float64)
        for b in range(B):
            n = yl[b]
            s = SO.frame_symbols(dur[b][:xl[b]], n)
            me, le = m_p[b:b + 1][:, :, s], logs_p[b:b + 1][:, :, s]                       # the prior expanded along the path
            zb, qb, mk = z_p[b:b + 1, :, :n], logs_q[b:b + 1, :, :n], torch.ones(1, 1, n)
            kl32[b] = kl_loss(zb, qb, me, le, mk) * mk.sum()
            d = lambda t: t.double()
            k = d(le) - d(qb) - 0.5
            k += 0.5 * ((d(zb) - d(me)) ** 2) * torch.exp(-2.0 * d(le))
            kl64[b] = torch.sum(k * d(mk))
        o64, frame64 = SO.kl_frames(z_p.double(), logs_q.double(), m_p.double(), logs_p.double(), dur, xl, yl)
        meta = dict(case=name, source="posterior_" + name + ".npz (z_p, logs_q64 as fp32, m_p, logs_p, durations)", torch=torch.__version__,
                    ref_err_kl=float((kl32.double() - kl64).abs().max()), oracle_vs_reference=float(((o64 - kl64).abs() / kl64.abs()).max()))
        path = os.path.join(out_dir, "score_kl_" + name + ".npz")
        np.savez_compressed(path, meta=json.dumps(meta), kl64=kl64.numpy(), kl_frame64=frame64.numpy())
        print(f"kl {name}: {os.path.getsize(path)} bytes; kl64 {kl64.tolist()} ref_err_kl {meta['ref_err_kl']:.3e} "
              f"restatement vs reference (rel) {meta['oracle_vs_reference']:.2e}")


if __name__ == "__main__":
    main()
