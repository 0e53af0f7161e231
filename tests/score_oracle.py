"""An independent torch restatement of what ``SynthesizerTrn.score`` computes, in the dtype of its inputs (fp64 for references, fp32 to
measure what fp32 arithmetic itself costs): the forward rational-quadratic spline with its log-determinant (reference
transforms.py:49-96, 188-208), the StochasticDurationPredictor run forward on observed durations (models.py:197-244) with every term
kept PER POSITION — the reference sums each over [1, 2] and returns a scalar per item; here the same terms are added position by
position, so ``nll_sym.sum(1)`` is the reference's ``nll + logq`` — and the KL term of losses.py:45-61 per frame along a path.
``tests/test_score_cpu.py`` holds it to the real reference's fp64 numbers (tests/golden/score_*.npz).  Test infrastructure."""
import math

import torch
import torch.nn.functional as F

from oracle.bv2_oracle import conv1x1, ddsconv

K = 10
TAIL = 5.0
LOG_2PI = math.log(2 * math.pi)


def _knots(u, lo, hi, min_size=1e-3):
    s = min_size + (1 - min_size * K) * torch.softmax(u, -1)
    c = F.pad(torch.cumsum(s, -1), (1, 0)) * (hi - lo) + lo
    c[..., 0], c[..., -1] = lo, hi
    return c, c[..., 1:] - c[..., :-1]


def rq_spline_forward(x, uw, uh, ud, tail=TAIL, min_d=1e-3):
    """x [...], uw / uh [..., K] (already divided by sqrt(filter_channels)), ud [..., K - 1] -> (y, logabsdet), both [...]; the identity
    with log-determinant 0 outside [-tail, tail]."""
    inside = (x >= -tail) & (x <= tail)
    ud = F.pad(ud, (1, 1), value=math.log(math.exp(1 - min_d) - 1))
    cw, w = _knots(uw, -tail, tail)
    ch, h = _knots(uh, -tail, tail)
    dv = min_d + F.softplus(ud)
    kn = cw.clone()
    kn[..., -1] += 1e-6
    xc = torch.where(inside, x, torch.zeros_like(x))
    b = ((xc[..., None] >= kn).sum(-1) - 1).clamp(0, K - 1)[..., None]
    pick = lambda t: t.gather(-1, b)[..., 0]
    icw, iw, ich, ih, idl, d0, d1 = pick(cw), pick(w), pick(ch), pick(h), pick(h / w), pick(dv), pick(dv[..., 1:])
    th = (xc - icw) / iw
    tomt = th * (1 - th)
    num = ih * (idl * th.pow(2) + d0 * tomt)
    den = idl + (d0 + d1 - 2 * idl) * tomt
    y = ich + num / den
    dnum = idl.pow(2) * (d1 * th.pow(2) + 2 * idl * tomt + d0 * (1 - th).pow(2))
    lad = torch.log(dnum) - 2 * torch.log(den)
    return torch.where(inside, y, x), torch.where(inside, lad, torch.zeros_like(lad))


def rq_spline_inverse(y, uw, uh, ud, tail=TAIL):
    from oracle.bv2_oracle import rq_spline_inverse as inv
    return inv(y, uw, uh, ud, tail)


def _convflow_forward(sd, p, z, mask, g):
    """modules.ConvFlow.forward, reverse=False: z [B, 2, T] -> (z, logabsdet * mask [B, T])"""
    x0, x1 = z[:, :1], z[:, 1:]
    fc = sd[p + ".pre.weight"].shape[0]
    h = ddsconv(sd, p + ".convs", conv1x1(sd, p + ".pre", x0), mask, 3, 3, g=g)
    h = (conv1x1(sd, p + ".proj", h) * mask).transpose(1, 2)
    y1, lad = rq_spline_forward(x1[:, 0], h[..., :K] / math.sqrt(fc), h[..., K:2 * K] / math.sqrt(fc), h[..., 2 * K:])
    return torch.cat([x0, y1[:, None]], 1) * mask, lad * mask[:, 0]


def _flows_forward(sd, prefix, z, mask, g):
    """ElementwiseAffine, then four (ConvFlow, Flip); returns z and the summed per-position log-determinant"""
    m, logs = sd[prefix + ".0.m"], sd[prefix + ".0.logs"]
    z = (m + torch.exp(logs) * z) * mask
    logdet = (logs * mask).sum(1)
    for f in (1, 3, 5, 7):
        z, ld = _convflow_forward(sd, f"{prefix}.{f}", z, mask, g)
        logdet = logdet + ld
        z = torch.flip(z, [1])
    return z, logdet


def sdp_forward(sd, x, x_mask, w, g, noise_e):
    """x [B, H, T], x_mask [B, 1, T], w [B, 1, T], g [B, gin, 1], noise_e [B, 2, T]; sd holds sdp.* including post_*.
    Returns (nll [B], nll_sym [B, T])."""
    h = conv1x1(sd, "sdp.pre", x) + conv1x1(sd, "sdp.cond", g)
    h = conv1x1(sd, "sdp.proj", ddsconv(sd, "sdp.convs", h, x_mask, 3, 3)) * x_mask
    hw = conv1x1(sd, "sdp.post_proj", ddsconv(sd, "sdp.post_convs", conv1x1(sd, "sdp.post_pre", w), x_mask, 3, 3)) * x_mask
    e_q = noise_e * x_mask
    z_q, logdet_q = _flows_forward(sd, "sdp.post_flows", e_q, x_mask, h + hw)
    z_u, z1 = z_q[:, :1], z_q[:, 1:]
    u = torch.sigmoid(z_u) * x_mask
    z0 = (w - u) * x_mask
    logdet_q = logdet_q + ((F.logsigmoid(z_u) + F.logsigmoid(-z_u)) * x_mask)[:, 0]
    logq = (-0.5 * (LOG_2PI + e_q ** 2) * x_mask).sum(1) - logdet_q
    y = torch.log(torch.clamp_min(z0, 1e-5)) * x_mask
    z, logdet = _flows_forward(sd, "sdp.flows", torch.cat([y, z1], 1), x_mask, h)
    logdet = logdet - y[:, 0]
    nll = (0.5 * (LOG_2PI + z ** 2) * x_mask).sum(1) - logdet
    sym = nll + logq
    return sym.sum(1), sym


def frame_symbols(durations, T_y):
    """durations [T] ints -> the symbol of frames 0 .. T_y - 1 (frames past the sum take the last symbol with a duration)"""
    d = torch.as_tensor(durations).long()
    idx = torch.repeat_interleave(torch.arange(len(d)), d)
    if len(idx) < T_y:
        idx = torch.cat([idx, idx[-1:].expand(T_y - len(idx))])
    return idx[:T_y]


def kl_frames(z_p, logs_q, m_p, logs_p, durations, x_lengths, y_lengths):
    """[B, C, Ty] x2, [B, C, T] x2, durations [B, T] -> (kl [B], kl_frame [B, Ty]) in the dtype of z_p"""
    B, C, Ty = z_p.shape
    out = torch.zeros(B, Ty, dtype=z_p.dtype)
    for b in range(B):
        n, tx = int(y_lengths[b]), int(x_lengths[b])
        s = frame_symbols(durations[b][:tx], n)
        m, lp = m_p[b][:, s], logs_p[b][:, s]
        kl = lp - logs_q[b][:, :n] - 0.5 + 0.5 * (z_p[b][:, :n] - m) ** 2 * torch.exp(-2.0 * lp)
        out[b, :n] = kl.sum(0)
    return out.sum(1), out
