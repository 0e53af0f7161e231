"""fp64 references of the BERT / DeBERTa-v2 feature extractor's own kernels (test infrastructure), each written from the operation's
definition: the disentangled attention of kernels/deberta_attn.hip, and the slab-summing LayerNorm and the embedding sum + LayerNorm
of kernels/bert.hip.  Also the cases and inputs the CPU proof (tests/test_bert_refs_cpu.py: the references against HuggingFace's
formulation, and the sensitivity of every case's inputs) and the GPU tests (tests/test_bert_kernels_gpu.py) share."""
import functools
import math

import torch

from oracle import deberta_oracle as DO

F64_MIN = torch.finfo(torch.float64).min


# ---------------------------------------------------------------------------------------------------------------- references
def ref_deberta_attention(q, k, v, pk, pq, tab, mask, P, index_shift=None, drop_c2p=False, drop_p2c=False):
    """q / k / v [B][H*D][T] (head h = rows h*D .. h*D + D - 1; every scale already folded into q and pq), pk / pq [H][D][2 span], tab
    [2P - 1] integers, mask [B][T] -> [B][H*D][T] in fp64:

        score[i][j] = Q_i.K_j + Q_i.PK[t(i - j)] + K_j.PQ[t(i - j)],   t(r) = tab[r + P - 1]

    pairs with a masked query or key set to the dtype's minimum, softmax over j, out_i = sum_j p[i][j] V_j.

    The keyword arguments exist for the sensitivity proofs alone (a deliberately WRONG result): index_shift [T][T] integers added to
    t(i - j) modulo 2 span; drop_c2p / drop_p2c leave the Q.PK / K.PQ term out."""
    B, HD, T = q.shape
    H, D, span2 = pk.shape
    assert HD == H * D and pq.shape == pk.shape and tab.numel() == 2 * P - 1 and T <= P
    q, k, v = [t.double().view(B, H, D, T).transpose(2, 3) for t in (q, k, v)]                 # [B][H][T][D]
    pk, pq = pk.double(), pq.double()
    i = torch.arange(T)
    idx = tab.long()[(i[:, None] - i[None, :]) + P - 1]                                         # [query i][key j]
    if index_shift is not None:
        idx = (idx + index_shift) % span2
    score = q @ k.transpose(-1, -2)
    if not drop_c2p:
        score = score + torch.gather(q @ pk, -1, idx.expand(B, H, T, T))                        # (Q_i.PK[r])[r = t(i - j)]
    if not drop_p2c:
        score = score + torch.gather(k @ pq, -1, idx.t().expand(B, H, T, T)).transpose(-1, -2)  # (K_j.PQ[r])[r = t(i - j)], laid out [j][i]
    pair = (mask[:, None, :, None] != 0) & (mask[:, None, None, :] != 0)
    score = score.masked_fill(~pair, F64_MIN)
    out = torch.softmax(score, -1) @ v
    return out.transpose(2, 3).reshape(B, HD, T)


def ref_bert_ln(slabs, gamma, beta, eps, mask=None):
    """slabs [nslab][B][C][T] -> LayerNorm over C (biased variance, eps inside the root) of their sum, times mask [B][T]."""
    x = slabs.double().sum(0)
    mean = x.mean(1, keepdim=True)
    var = ((x - mean) ** 2).mean(1, keepdim=True)
    y = (x - mean) / torch.sqrt(var + eps) * gamma.double()[None, :, None] + beta.double()[None, :, None]
    return y if mask is None else y * mask.double()[:, None, :]


def ref_bert_embed_ln(input_ids, token_type_ids, word, pos, typ, lengths, gamma, beta, eps):
    """LayerNorm_C(word[clamp(id)] + typ[clamp(tt)] + pos[min(s, max_pos - 1)]) as [B][C][S]; token_type_ids / pos / typ / lengths
    may be None (type 0 / no such table / nothing zeroed); columns s >= lengths[b] are zero."""
    B, S = input_ids.shape
    x = word.double()[input_ids.clamp(0, word.shape[0] - 1)]
    if typ is not None:
        tt = torch.zeros_like(input_ids) if token_type_ids is None else token_type_ids
        x = x + typ.double()[tt.clamp(0, typ.shape[0] - 1)]
    if pos is not None:
        x = x + pos.double()[torch.arange(S).clamp(max=pos.shape[0] - 1)][None]
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    y = (x - mean) / torch.sqrt(var + eps) * gamma.double() + beta.double()
    if lengths is not None:
        y = y * (torch.arange(S)[None, :] < lengths[:, None]).double()[..., None]
    return y.transpose(1, 2)


def masked_rel_err(got, ref, mask):
    """The error measure of tests/test_kernels_gpu.py: max-abs error over the valid (unmasked) columns / the reference's max-abs."""
    valid = (mask != 0)[:, None, :].expand_as(ref)
    return ((got.double().cpu() - ref).abs()[valid].max() / ref.abs().max()).item()


# ---------------------------------------------------------------------------------------------------------------- DeBERTa cases
def linear_table(P, span):
    """The table of a model without buckets (position_buckets <= 0: bucket(r) = r): slope 1 everywhere, saturating at both ends when
    span < P."""
    return torch.clamp(torch.arange(-(P - 1), P) + span, 0, 2 * span - 1)


# name -> (table, B, H, D, T, lengths, seed).  table: "LARGE_V3" (P 512, span 256, log spacing beyond |r| 128) / "MID_V3" (P 160, span 32,
# log spacing beyond 16) from oracle.deberta_oracle.relative_index_table, or ("linear", P, span)
DEBERTA_CASES = {
    "real_config":        ("LARGE_V3", 2, 2, 64, 300, (300, 161), 1),      # 10 key tiles: the loop with the alpha rescale, the log region
    "mid_h3_d32":         ("MID_V3", 2, 3, 32, 160, (160, 97), 2),         # T = P
    "mid_h1_d96":         ("MID_V3", 2, 1, 96, 160, (160, 97), 3),
    "mid_h2_d128":        ("MID_V3", 2, 2, 128, 160, (160, 97), 4),
    "large_h1_d128":      ("LARGE_V3", 2, 1, 128, 300, (300, 161), 5),     # 153.6 KB of LDS
    "large_h4_d32":       ("LARGE_V3", 2, 4, 32, 300, (300, 161), 6),
    "t512":               ("LARGE_V3", 1, 1, 64, 512, (512,), 7),          # T = P: table entries 0 and 2P - 2
    "t1":                 ("LARGE_V3", 1, 2, 64, 1, (1,), 8),
    "t32":                ("LARGE_V3", 1, 2, 64, 32, (32,), 9),
    "t33_ragged":         ("LARGE_V3", 3, 2, 64, 33, (33, 1, 2), 10),
    "t129":               ("LARGE_V3", 2, 2, 64, 129, (129, 128), 11),
    "nobucket_t64":       (("linear", 64, 64), 2, 2, 64, 64, (64, 41), 12),   # every tile pair: two 32-row blocks, all 63 staged rows
    "nobucket_t50":       (("linear", 64, 64), 2, 2, 64, 50, (50, 17), 13),
    "nobucket_d128":      (("linear", 64, 64), 2, 2, 128, 64, (64, 41), 14),
    "span8":              (("linear", 64, 8), 2, 2, 64, 64, (64, 20), 15),    # 2 span = 16 < 32 staged rows; saturates at both ends
}


def deberta_table(table):
    """-> (tab int64 [2P - 1], P, span, half): half = the |i - j| beyond which perturbation (a) of the sensitivity proof acts — the
    bucket midpoint (position_buckets / 2: where the log spacing starts), span / 2 for a table without buckets."""
    if isinstance(table, str):
        cfg = getattr(DO, table)
        P, span = cfg["max_position_embeddings"], DO.att_span(cfg)
        return DO.relative_index_table(cfg, P), P, span, cfg["position_buckets"] // 2
    _, P, span = table
    return linear_table(P, span), P, span, span // 2


@functools.lru_cache(maxsize=None)
def deberta_case(name):
    """The inputs of a case (fp32, fixed seed) and its fp64 reference, computed once per process and never modified.  Entries of q (after
    the fold of 1 / sqrt(3 D)), k, pk and pq are N(0, 1.5^2 / sqrt(D)), so each of the three score terms is a sum of D products of
    variance 1.5^4 / D: standard deviation 2.25 each; v is N(0, 1)."""
    table, B, H, D, T, lens, seed = DEBERTA_CASES[name]
    tab, P, span, half = deberta_table(table)
    g = torch.Generator().manual_seed(1000 + seed)
    sd = 1.5 / D ** 0.25
    q, k = torch.randn(B, H * D, T, generator=g) * sd, torch.randn(B, H * D, T, generator=g) * sd
    v = torch.randn(B, H * D, T, generator=g)
    pk, pq = torch.randn(H, D, 2 * span, generator=g) * sd, torch.randn(H, D, 2 * span, generator=g) * sd
    mask = (torch.arange(T)[None, :] < torch.tensor(lens)[:, None]).float()
    ref = ref_deberta_attention(q, k, v, pk, pq, tab, mask, P)
    return dict(B=B, H=H, D=D, T=T, P=P, span=span, half=half, tab=tab, q=q, k=k, v=v, pk=pk, pq=pq, mask=mask, ref=ref)


# ---------------------------------------------------------------------------------------------------------------- W = 0 attention cases
# (B, T, lens, H, D): plain multi-head attention as BERT runs it through kernels/attention.hip — window 0: one band logit row per head
# (the diagonal's) and one relative-value row
W0_CASES = [(1, 53, (53,), 16, 64), (1, 53, (53,), 4, 32), (2, 300, (300, 129), 16, 64), (2, 300, (300, 129), 4, 32)]
ERV_SD = 2.0      # the relative-value row against v's N(0, 1): dropping it must be seen at 100 x the fp16 form's bar as well


@functools.lru_cache(maxsize=None)
def w0_case(B, T, lens, H, D, W=0):
    """-> (qkv [B][3HD][T] with UNSCALED q rows as tests.encoder_refs.ref_attention takes them, erk, erv [2W + 1][D], mask, ref): the
    scaled q, k and erk are N(0, 1.5^2 / sqrt(D)) (content and band logits of standard deviation 2.25), v N(0, 1), erv N(0, ERV_SD^2)."""
    from tests.encoder_refs import ref_attention
    g = torch.Generator().manual_seed(77 + T + 7 * H + D + 1000 * W)
    sd = 1.5 / D ** 0.25
    qkv = torch.randn(B, 3 * H * D, T, generator=g)
    qkv[:, : H * D] *= sd * math.sqrt(D)
    qkv[:, H * D: 2 * H * D] *= sd
    erk = torch.randn(2 * W + 1, D, generator=g) * sd
    erv = torch.randn(2 * W + 1, D, generator=g) * ERV_SD
    mask = (torch.arange(T)[None, :] < torch.tensor(lens)[:, None]).float()
    return qkv, erk, erv, mask, ref_attention(qkv, mask, erk, erv, H, W)
