"""fp64 references of the Encoder layer's operations for the kernel-level tests (test infrastructure): the windowed
relative-position attention in the unsplit form of kernels/attention.hip's header, conv_o, the channel LayerNorm, and the
flash-decoding merge of key ranges written out from its definition.  tests/test_encoder_forms_cpu.py holds them to the oracle."""
import math

import torch


def ref_attention(qkv, mask, erk, erv, H, W):
    B, C3, T = qkv.shape
    HD = C3 // 3
    D = HD // H
    q, k, v = [t.view(B, H, D, T).transpose(2, 3).double() for t in qkv.split(HD, 1)]
    qs = q / math.sqrt(D)
    s = qs @ k.transpose(-1, -2)
    idx = torch.arange(T)
    rel = idx[None, :] - idx[:, None]
    band = rel.abs() <= W
    ql = qs @ erk.double().t()
    s = s + torch.where(band, ql.gather(-1, (rel + W).clamp(0, 2 * W).expand(B, H, T, T)), torch.zeros((), dtype=torch.float64))
    pair = (mask[:, None, :, None] * mask[:, None, None, :]) != 0
    s = torch.where(pair, s, torch.full((), -1e4, dtype=torch.float64))
    p = torch.softmax(s, -1)
    o = p @ v
    relw = torch.zeros(B, H, T, 2 * W + 1, dtype=torch.float64)
    for r in range(-W, W + 1):
        lo, hi = max(0, -r), min(T, T - r)
        if hi > lo:
            i = torch.arange(lo, hi)
            relw[:, :, lo:hi, r + W] = p[:, :, i, i + r]
    o = o + relw @ erv.double()
    return o.transpose(2, 3).reshape(B, HD, T)


def ref_logits(qkv, mask, erk, H, W):
    """The logits [B][H][query][key] of ref_attention (masked pairs SET to -1e4), for the per-range statistics."""
    B, C3, T = qkv.shape
    HD = C3 // 3
    D = HD // H
    q, k = [t.view(B, H, D, T).transpose(2, 3).double() for t in qkv.split(HD, 1)[:2]]
    qs = q / math.sqrt(D)
    s = qs @ k.transpose(-1, -2)
    ql = qs @ erk.double().t()
    for r in range(-W, W + 1):                                        # key j = i + r
        i = torch.arange(max(0, -r), min(T, T - r))
        s[:, :, i, i + r] += ql[:, :, i, r + W]
    pair = (mask[:, None, :, None] * mask[:, None, None, :]) != 0
    return torch.where(pair, s, torch.full((), -1e4, dtype=torch.float64))


def key_ranges(T, ks):
    """The key split's rule: range r owns the 32-key tiles [n r / ks, n (r + 1) / ks) of the n = ceil(T / 32) tiles."""
    n = (T + 31) // 32
    return [(min(T, 32 * (n * r // ks)), min(T, 32 * (n * (r + 1) // ks))) for r in range(ks)]


def ref_attention_range(qkv, erv, H, W, k0, k1, logits):
    """Attention over the keys [k0, k1) alone (logits = ref_logits(...)): softmax normalised over that range, relative-value terms
    of the range's keys only.  Returns (out [B][HD][T], m [B][H][T], l [B][H][T]): the range's logit max and sum of
    exp(logit - m) per query."""
    B, C3, T = qkv.shape
    HD = C3 // 3
    D = HD // H
    v = qkv[:, 2 * HD:].view(B, H, D, T).transpose(2, 3).double()
    s = logits[..., k0:k1]
    m = s.max(-1).values
    e = torch.exp(s - m[..., None])
    l = e.sum(-1)
    p = e / l[..., None]
    o = p @ v[:, :, k0:k1]
    ev = erv.double()
    for r in range(-W, W + 1):                                        # key j = i + r inside [k0, k1)
        i = torch.arange(max(0, k0 - r), min(T, k1 - r))
        if len(i):
            o[:, :, i] += p[:, :, i, i + r - k0, None] * ev[r + W]
    return o.transpose(2, 3).reshape(B, HD, T), m, l


def ref_conv_o(att, wo, bo=None, res=None):
    """conv_o (1x1): att [B][HD][T], wo [Co][HD] -> [B][Co][T] (+ bias, + residual)."""
    y = torch.einsum("oc,bct->bot", wo.double(), att.double())
    if bo is not None:
        y = y + bo.double()[None, :, None]
    if res is not None:
        y = y + res.double()
    return y


def ref_layer_norm(x, gamma, beta, eps=1e-5, with_rstd=False):
    """LayerNorm over the channels of [B][C][T]: biased variance, eps inside the root."""
    x = x.double()
    mean = x.mean(1, keepdim=True)
    var = ((x - mean) ** 2).mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    y = (x - mean) * rstd * gamma.double()[None, :, None] + beta.double()[None, :, None]
    return (y, rstd) if with_rstd else y


def ref_ln_vec_mask(x, gamma, beta, vec=None, mask=None, eps=1e-5):
    """(LN(x) + vec[b][c]) * mask[b][t]"""
    y = ref_layer_norm(x, gamma, beta, eps)
    if vec is not None:
        y = y + vec.double()[:, :, None]
    if mask is not None:
        y = y * mask.double()[:, None, :]
    return y


def ref_split_merge(slabs, m, l):
    """slabs [H][ks][B][C][T] (range r of head h, normalised over the range alone), m / l [B][H][ks][T] -> sum over the heads of
    sum_r w_r slab_r with w_r = l_r e^{m_r - M} / sum_r' l_r' e^{m_r' - M}, M = max_r m_r: [B][C][T]."""
    H, ks = slabs.shape[:2]
    out = torch.zeros(slabs.shape[2:], dtype=torch.float64)
    m, l = m.double(), l.double()
    for h in range(H):
        M = m[:, h].max(1).values                                     # [B][T]
        num = [l[:, h, r] * torch.exp(m[:, h, r] - M) for r in range(ks)]
        den = sum(num)
        for r in range(ks):
            out += (num[r] / den)[:, None, :] * slabs[h, r].double()
    return out


# ---- the cases of the key-split tests, shared by the CPU proof of the references and the GPU tests
# (B, T, lens, H, D, ks, q multiplier)
SPLIT_CASES = [
    (1, 65, (65,), 2, 96, 2, 3.0),             # 3 tiles, the last with one key
    (1, 65, (65,), 4, 32, 2, 3.0),
    (1, 160, (160,), 1, 128, 4, 3.0),          # ranges of 1, 1, 1, 2 tiles
    (1, 160, (160,), 2, 96, 4, 3.0),
    (1, 384, (384,), 2, 96, 4, 3.0),           # the product's shape
    (1, 384, (384,), 4, 32, 2, 3.0),
    (1, 600, (600,), 2, 128, 2, 3.0),          # ranges of 9 and 10 tiles: the looping variants under a non-zero first tile
    (1, 600, (600,), 2, 96, 2, 3.0),
    (2, 256, (256, 40), 2, 96, 4, 3.0),        # ragged: ranges 2 and 3 of item 1 are fully masked for its valid queries
    (2, 256, (256, 40), 1, 64, 4, 3.0),
    (1, 160, (160,), 2, 96, 4, 12.0),          # peaked
    (1, 384, (384,), 1, 96, 4, 12.0),
]
WINDOW = 4


def attention_inputs(B, T, lens, H, D, qmul=3.0, seed=None):
    """Random q/k/v rows [B][3HD][T] (q multiplied by qmul: sharpens the softmax), relative embeddings, mask."""
    g = torch.Generator().manual_seed(T + 7 * H + D if seed is None else seed)
    qkv = torch.randn(B, 3 * H * D, T, generator=g)
    qkv[:, : H * D] *= qmul
    erk = torch.randn(2 * WINDOW + 1, D, generator=g) * D ** -0.5
    erv = torch.randn(2 * WINDOW + 1, D, generator=g) * D ** -0.5
    mask = (torch.arange(T)[None, :] < torch.tensor(lens)[:, None]).float()
    return qkv, erk, erv, mask


def conv_o_weights(H, D, Co, B, T, seed=1):
    g = torch.Generator().manual_seed(seed + 13 * H + D + Co)
    wo = torch.randn(Co, H * D, generator=g) / math.sqrt(H * D)
    return wo, torch.randn(Co, generator=g), torch.randn(B, Co, T, generator=g)
