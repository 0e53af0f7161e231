"""Generate ``tests/golden/align_*.npz``: the REAL reference's forward flow and negative cross-entropy matrix — build-container only.

    python tools/gen_align_golden.py          # from the repo root, needs the reference checkout (oracle.ref_import)

The reference's aligner lives inside ``SynthesizerTrn.forward()`` (models.py:954-991): ``enc_p``, ``enc_q``, ``flow(z, y_mask, g=g)`` in the
forward direction, the four-term ``neg_cent`` and ``monotonic_align.maximum_path``.  This tool runs that method as it is and takes its
intermediates out of it, copying nothing:

* a forward hook on ``enc_q`` replaces its output with a given latent ``z`` (seeded noise times the frame mask — the posterior encoder is
  not part of this library, and with synthetic weights its output would be noise of the same kind), so the flow runs on a known input;
* a forward hook on ``flow`` records ``z_p``, one on ``enc_p`` records ``m_p`` / ``logs_p`` / ``x_mask``;
* ``monotonic_align`` is a stub here (numba is absent): its ``maximum_path`` receives the reference's own fp32 ``neg_cent``, records it
  and ends the call — the losses behind it are out of scope.  ``use_noise_scaled_mas`` is switched off on the instance: the matrix is
  the deterministic one of models.py:962-975.

Every case is run in fp32 and once more with the whole module in ``.double()`` on the same fp32-valued inputs: ``z_p64`` is the flow's
fp64 result, and ``ref_err_z_p = max|z_p - z_p64|`` the reference's own fp32 error, from which the GPU test builds its bar.  For the matrix
the fp64 value is the definition evaluated on the fixture's fp32 ``z_p`` / ``m_p`` / ``logs_p`` (tests/posterior_oracle.py ``neg_cent_f64``):
``ref_err_neg_cent`` is the reference's fp32 error against that.  The path (``durations``, ``score``) is the fp32 numpy restatement of the
dynamic programme on the reference's matrix.

Cases: ``narrow_b2_t18`` (transformer flow, 3 couplings: the odd count, inter 128), ``mix_b2_ragged`` (the v2.3 widths, 4 couplings) and
``wn_b1_t16`` (the WN flow).  Weights come from the case's seed and are not stored.
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bert_vits2_amd import synth  # noqa: E402
from oracle import cases, ref_import  # noqa: E402
from tests import posterior_oracle as PO  # noqa: E402

CASES = {"narrow_b2_t18": [52, 40], "mix_b2_ragged": [64, 47], "wn_b1_t16": [48]}      # frames per item
Z_SEED = 8642


class _Captured(Exception):
    pass


def latent(B, C, y_lengths):
    g = torch.Generator().manual_seed(Z_SEED)
    Ty = max(y_lengths)
    z = torch.randn(B, C, Ty, generator=g)
    mask = (torch.arange(Ty)[None, :] < torch.tensor(y_lengths)[:, None]).float()[:, None, :]
    return z * mask, mask


@torch.no_grad()
def run_forward(net, hp, batch, z, y_mask, y_lengths, dtype):
    """The reference's forward() up to maximum_path, with the hooks described above."""
    taps = {}
    cast = lambda t: t.to(dtype) if torch.is_floating_point(t) else t
    zq, ym = cast(z), cast(y_mask)
    hooks = [net.enc_q.register_forward_hook(lambda mod, inp, out: (zq, zq, torch.zeros_like(zq), ym)),
             net.flow.register_forward_hook(lambda mod, inp, out: taps.__setitem__("z_p", out)),
             net.enc_p.register_forward_hook(lambda mod, inp, out: taps.__setitem__("enc_p", out))]

    def stub(neg_cent, mask):
        taps["neg_cent"] = neg_cent.detach().clone()
        taps["attn_mask"] = mask.detach().clone()
        raise _Captured()

    ma = sys.modules["monotonic_align"]
    ma.maximum_path = stub
    net.use_noise_scaled_mas = False                                # models.py:976-982: a training-time perturbation of the matrix, out of scope
    B, Ty = z.shape[0], z.shape[2]
    y = torch.zeros(B, hp.spec_channels, Ty, dtype=dtype)           # enc_q's own input: its output is replaced
    try:
        net.forward(batch["x"], batch["x_lengths"], y, torch.tensor(y_lengths), batch["sid"], batch["tone"], batch["language"],
                    cast(batch["bert"]), cast(batch["ja_bert"]), cast(batch["en_bert"]))
        raise RuntimeError("forward() did not reach maximum_path")
    except _Captured:
        pass
    finally:
        for h in hooks:
            h.remove()
        del ma.maximum_path
    return taps


def main():
    torch.set_num_threads(1)
    torch.use_deterministic_algorithms(True)
    out_dir = os.path.join(ROOT, "tests", "golden")
    for name, y_lengths in CASES.items():
        hp, seed, batch, _nw, _nz, _kw = cases.build_case(name)
        sd = synth.synthetic_state_dict(hp, seed)
        B = batch["x"].shape[0]
        x_lengths = batch["x_lengths"].tolist()
        z, y_mask = latent(B, hp.inter_channels, y_lengths)
        torch.manual_seed(0)                                         # enc_q's unused weights: initialised the same way in both builds
        t32 = run_forward(ref_import.build_reference_net(hp, sd), hp, batch, z, y_mask, y_lengths, torch.float32)
        torch.manual_seed(0)
        t64 = run_forward(ref_import.build_reference_net(hp, sd).double(), hp, batch, z, y_mask, y_lengths, torch.float64)
        _x, m_p, logs_p, x_mask = t32["enc_p"]
        z_p, z_p64, nc = t32["z_p"], t64["z_p"], t32["neg_cent"]
        assert z_p.dtype == torch.float32 and z_p64.dtype == torch.float64 and nc.dtype == torch.float32
        assert torch.equal(t32["attn_mask"].sum(2)[:, 0].long(), batch["x_lengths"]) and t32["attn_mask"].sum(1)[:, 0].long().tolist() == y_lengths
        nc64 = PO.neg_cent_f64(z_p.numpy(), m_p.numpy(), logs_p.numpy())
        err_nc = float(np.abs(nc.double().numpy() - nc64).max())
        err_zp = float((z_p.double() - z_p64).abs().max())
        ncm = nc.numpy().copy()                                      # the matrix the device writes: zeros outside the lengths
        for b in range(B):
            ncm[b, y_lengths[b]:, :] = 0
            ncm[b, :, x_lengths[b]:] = 0
        dur, _attn, score = PO.maximum_path(ncm, x_lengths, y_lengths)
        arr = dict(z=z.numpy(), z_p=z_p.numpy(), z_p64=z_p64.numpy(), m_p=m_p.numpy(), logs_p=logs_p.numpy(), x_mask=x_mask.numpy(),
                   neg_cent=ncm, durations=dur, score=score, y_lengths=np.asarray(y_lengths, dtype=np.int64),
                   x_lengths=np.asarray(x_lengths, dtype=np.int64))
        meta = dict(case=name, seed=seed, z_seed=Z_SEED, y_lengths=y_lengths, x_lengths=x_lengths, torch=torch.__version__,
                    checksums=cases.weight_checksums(sd), ref_err_z_p=err_zp, ref_err_neg_cent=err_nc,
                    z_p_absmax=float(z_p64.abs().max()), neg_cent_absmax=float(np.abs(nc64).max()),
                    note="z_p = reference flow(z, y_mask, g) forward in fp32, z_p64 the same module in fp64; neg_cent = the reference's "
                         "models.py:962-975 in fp32 (zeroed outside the lengths); durations / score = tests/posterior_oracle.py on it")
        path = os.path.join(out_dir, "align_" + name + ".npz")
        np.savez_compressed(path, meta=json.dumps(meta), **arr)
        print(f"{name}: {os.path.getsize(path)} bytes  ref_err z_p {err_zp:.3e} (|z_p| max {meta['z_p_absmax']:.2f})  "
              f"ref_err neg_cent {err_nc:.3e} (|neg_cent| max {meta['neg_cent_absmax']:.1f})  durations {dur.tolist()}")


if __name__ == "__main__":
    main()
