"""Generate ``tests/golden/posterior_*.npz``: the REAL reference's PosteriorEncoder, forward flow, ``neg_cent`` and path — build-container only.

    python tools/gen_posterior_golden.py      # from the repo root, needs the reference checkout (oracle.ref_import)

The reference's own ``SynthesizerTrn.forward()`` is run up to ``monotonic_align.maximum_path`` (the machinery of ``tools/gen_align_golden.py``:
forward hooks record ``enc_p`` / ``enc_q`` / ``flow``, the ``monotonic_align`` stub records the fp32 ``neg_cent`` and ends the call,
``use_noise_scaled_mas`` is off) — here with NOTHING replaced: ``enc_q`` runs on a spectrogram with its own weights
(``synth.synthetic_posterior_state_dict``), and the one draw of models.py:486 (``torch.randn_like(m)``) is handed a stored ``noise_q``.
Every case runs in fp32 and once more with the module in ``.double()`` on the same inputs; ``ref_err_<t>`` = max|fp32 - fp64| per tensor
(``m_q``, ``logs_q``, ``z``, ``z_p``) is the reference's own fp32 error, from which the GPU test builds its 4 x bars.  The path is the fp32
numpy restatement (tests/posterior_oracle.py) on the reference's matrix.

Cases, each B = 2 ragged where the model case is: ``narrow_b2_t18`` with ``spec_channels = 80`` (3 couplings), ``mix_b2_ragged`` at the v2.3
widths with ``spec_channels = 1025`` (transformer flow), ``wn_b1_t16`` with 1025 (WN flow).  The spectrograms are rebuilt by the tests from
the metadata (``synth.synthetic_reference_spec(spec, L, index)``), the weights from the seeds; ``noise_q`` is stored.
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bert_vits2_amd import hparams as H, synth  # noqa: E402
from oracle import cases, ref_import  # noqa: E402
from tests import posterior_oracle as PO  # noqa: E402
from gen_align_golden import _Captured  # noqa: E402

CASES = {"narrow_b2_t18": dict(spec=80, frames=[52, 40]), "mix_b2_ragged": dict(spec=1025, frames=[64, 47]),
         "wn_b1_t16": dict(spec=1025, frames=[48])}
NOISE_SEED = 1357


def case_hparams(name):
    return H.default_v23(**dict(cases.CASES[name]["hp"], spec_channels=CASES[name]["spec"]))


def spectrogram(spec, frames):
    """[B, spec, max(frames)]: item b is synthetic_reference_spec(spec, frames[b], b), zero-padded."""
    y = torch.zeros(len(frames), spec, max(frames))
    for b, L in enumerate(frames):
        y[b, :, :L] = synth.synthetic_reference_spec(spec, L, b)
    return y


@torch.no_grad()
def run_forward(net, batch, y, y_lengths, noise_q, dtype):
    taps = {}
    cast = lambda t: t.to(dtype) if torch.is_floating_point(t) else t
    hooks = [net.enc_q.register_forward_hook(lambda mod, inp, out: taps.__setitem__("enc_q", out)),
             net.flow.register_forward_hook(lambda mod, inp, out: taps.__setitem__("z_p", out)),
             net.enc_p.register_forward_hook(lambda mod, inp, out: taps.__setitem__("enc_p", out))]

    def stub(neg_cent, mask):
        taps["neg_cent"] = neg_cent.detach().clone()
        raise _Captured()

    ma = sys.modules["monotonic_align"]
    ma.maximum_path = stub
    net.use_noise_scaled_mas = False
    real_like, draws = torch.randn_like, []

    def fake_like(t, **kw):
        assert tuple(t.shape) == tuple(noise_q.shape), (t.shape, noise_q.shape)
        draws.append(1)
        return noise_q.to(t.dtype).clone()

    torch.randn_like = fake_like
    try:
        net.forward(batch["x"], batch["x_lengths"], cast(y), torch.tensor(y_lengths), batch["sid"], batch["tone"], batch["language"],
                    cast(batch["bert"]), cast(batch["ja_bert"]), cast(batch["en_bert"]))
        raise RuntimeError("forward() did not reach maximum_path")
    except _Captured:
        pass
    finally:
        torch.randn_like = real_like
        for h in hooks:
            h.remove()
        del ma.maximum_path
    assert len(draws) == 1, "exactly the draw of models.py:486 is expected before maximum_path"
    return taps


def main():
    torch.set_num_threads(1)
    torch.use_deterministic_algorithms(True)
    out_dir = os.path.join(ROOT, "tests", "golden")
    for name, cs in CASES.items():
        hp = case_hparams(name)
        base = cases.CASES[name]
        seed = base["seed"]
        batch = synth.synthetic_batch(base["lengths"], base["languages"], base["sids"])
        sd = synth.synthetic_state_dict(hp, seed)
        sd.update(synth.synthetic_posterior_state_dict(hp, seed))
        frames, B = cs["frames"], len(cs["frames"])
        x_lengths = batch["x_lengths"].tolist()
        y = spectrogram(hp.spec_channels, frames)
        noise_q = torch.randn(B, hp.inter_channels, max(frames), generator=torch.Generator().manual_seed(NOISE_SEED))
        t32 = run_forward(ref_import.build_reference_net(hp, sd), batch, y, frames, noise_q, torch.float32)
        t64 = run_forward(ref_import.build_reference_net(hp, sd).double(), batch, y, frames, noise_q, torch.float64)
        z, m_q, logs_q, y_mask = t32["enc_q"]
        z64, m64, l64, _ = t64["enc_q"]
        _x, m_p, logs_p, x_mask = t32["enc_p"]
        z_p, z_p64, nc = t32["z_p"], t64["z_p"], t32["neg_cent"]
        assert z.dtype == torch.float32 and z64.dtype == torch.float64 and y_mask.sum([1, 2]).long().tolist() == frames
        err = lambda a, b: float((a.double() - b).abs().max())
        nc64 = PO.neg_cent_f64(z_p.numpy(), m_p.numpy(), logs_p.numpy())
        ncm = nc.numpy().copy()
        for b in range(B):
            ncm[b, frames[b]:, :] = 0
            ncm[b, :, x_lengths[b]:] = 0
        dur, _attn, score = PO.maximum_path(ncm, x_lengths, frames)
        arr = dict(noise_q=noise_q.numpy(), z64=z64.numpy(),      # the fp32 m_q / logs_q / z are in the ref_err figures only: each file stays under 1 MiB
                   m_q64=m64.numpy(),
                   logs_q64=l64.numpy(), z_p=z_p.numpy(), z_p64=z_p64.numpy(), m_p=m_p.numpy(), logs_p=logs_p.numpy(), neg_cent=ncm,
                   durations=dur, score=score, y_lengths=np.asarray(frames, dtype=np.int64), x_lengths=np.asarray(x_lengths, dtype=np.int64))
        meta = dict(case=name, seed=seed, spec_channels=hp.spec_channels, frames=frames, x_lengths=x_lengths, noise_seed=NOISE_SEED,
                    torch=torch.__version__, checksums=cases.weight_checksums(sd),
                    ref_err_m_q=err(m_q, m64), ref_err_logs_q=err(logs_q, l64), ref_err_z=err(z, z64), ref_err_z_p=err(z_p, z_p64),
                    ref_err_neg_cent=float(np.abs(nc.double().numpy() - nc64).max()),
                    absmax=dict(m_q=float(m64.abs().max()), logs_q=float(l64.abs().max()), z=float(z64.abs().max()), z_p=float(z_p64.abs().max())),
                    note="the reference's forward() up to maximum_path, fp32 and fp64 (the *64 arrays); neg_cent zeroed outside the lengths")
        path = os.path.join(out_dir, "posterior_" + name + ".npz")
        np.savez_compressed(path, meta=json.dumps(meta), **arr)
        print(f"{name}: {os.path.getsize(path)} bytes; ref_err m_q {meta['ref_err_m_q']:.3e} logs_q {meta['ref_err_logs_q']:.3e} z {meta['ref_err_z']:.3e} "
              f"z_p {meta['ref_err_z_p']:.3e} neg_cent {meta['ref_err_neg_cent']:.3e}; absmax {meta['absmax']}; durations {dur.tolist()}")


if __name__ == "__main__":
    main()
