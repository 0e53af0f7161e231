"""fp64 restatements of the fp32 WN layer's two launches (bv2_exec.cpp run_wn; reference modules.py:185-210, commons.py:98-105), the
packer's row permutation in Python, deliberately wrong variants of each for the discrimination test, and the inputs the GPU tests use
(tests/test_wn_forms_cpu.py checks the restatements and the inputs on the CPU, tests/test_wn_forms_gpu.py holds the kernels to them).

Row orders.  "Reference order": in_layer row c < H is channel c's tanh row, row H + c its sigmoid row.  "Gate order" (what the kernels
read): every 32-row tile holds the tanh rows of 16 channels, then the sigmoid rows of the same 16."""
import functools
import math

import torch
import torch.nn.functional as F

K = 5                     # the only WN conv the product builds: kernel 5, dilation 1
BAR = 2e-5                # both bars of the GPU tests: |err| <= BAR * max|v| (gate), rel_err < BAR (res_skip)


# ---------------------------------------------------------------------------------------------------------------- the permutation
def gate_row(H, n):
    """Source (reference-order) row of gate-order row n of a 2H-row in_layer or conditioning slice."""
    mt, j = divmod(n, 32)
    return 16 * mt + j if j < 16 else H + 16 * mt + (j - 16)


def gate_perm(H):
    return torch.tensor([gate_row(H, n) for n in range(2 * H)], dtype=torch.long)


# ---------------------------------------------------------------------------------------------------------------- the launches
def gate(v, H):
    """v [B][2H][L] in reference order -> [B][H][L]."""
    return torch.tanh(v[:, :H]) * torch.sigmoid(v[:, H:])


def gate_packed(v):
    """v [B][2H][L] in gate order -> [B][H][L] in natural channel order."""
    B, R, L = v.shape
    v5 = v.reshape(B, R // 32, 2, 16, L)
    return (torch.tanh(v5[:, :, 0]) * torch.sigmoid(v5[:, :, 1])).reshape(B, R // 2, L)


def preact(x, w, b, gl):
    """conv + bias + g_l, all fp64: x [B][H][L], w [2H][H][K], b [2H], gl [B][2H]; rows stay in the order they are given."""
    return F.conv1d(x.double(), w.double(), b.double(), padding=(K - 1) // 2) + gl.double()[:, :, None]


def in_layer(x, w, b, gl):
    return gate(preact(x, w, b, gl), w.shape[0] // 2)


def res_skip(acts, w, b, x, outacc, mask, first, last):
    """-> (x, outacc) after the launch.  mask [B][L]; outacc is ignored when first."""
    H = acts.shape[1]
    m = mask.double()[:, None, :]
    rs = F.conv1d(acts.double(), w.double(), b.double())
    prev = 0.0 if first else outacc.double()
    if last:
        return x.double(), (prev + rs) * m
    return (x.double() + rs[:, :H]) * m, prev + rs[:, H:]


def cond(g, cw, cb):
    """cond_layer: g [B][gin] -> [B][2H * layers]."""
    return F.conv1d(g.double()[:, :, None], cw.double(), cb.double())[:, :, 0]


def chain(x, gl_all, mask, ins, rss):
    """The layers one after the other: ins / rss = [(w, b)] per layer.  Returns per layer the dict of its launches' inputs and outputs
    (x_in, acts, out_in, x_out, out), all fp64; the last entry's `out` is WN.forward's result."""
    H, n = x.shape[1], len(ins)
    x, out, steps = x.double(), None, []
    for i in range(n):
        acts = in_layer(x, ins[i][0], ins[i][1], gl_all[:, 2 * H * i:2 * H * (i + 1)])
        xn, on = res_skip(acts, rss[i][0], rss[i][1], x, out, mask, i == 0, i == n - 1)
        steps.append(dict(x_in=x, acts=acts, out_in=out, x_out=xn, out=on))
        x, out = xn, on
    return steps


# ---------------------------------------------------------------------------------------------------------------- wrong on purpose
def gate_halves_swapped(v, H):
    return torch.tanh(v[:, H:]) * torch.sigmoid(v[:, :H])


def gate_packed_halves_swapped(v):
    B, R, L = v.shape
    v5 = v.reshape(B, R // 32, 2, 16, L)
    return (torch.tanh(v5[:, :, 1]) * torch.sigmoid(v5[:, :, 0])).reshape(B, R // 2, L)


def gl_item0(gl):
    return gl[:1].expand_as(gl)


def gl_unpermuted(gl, H):
    """What reference-order row r sees when the weights are permuted and g_l is not: packed row n = gate_row^-1(r) reads gl[n]."""
    inv = torch.empty(2 * H, dtype=torch.long)
    inv[gate_perm(H)] = torch.arange(2 * H)
    return gl[:, inv]


def res_skip_rows_from_res(acts, w, b, x, outacc, mask, first):
    H = acts.shape[1]
    rs = F.conv1d(acts.double(), w.double(), b.double())
    return (0.0 if first else outacc.double()) + rs[:, :H]


def res_skip_add_after_mask(acts, w, b, x, outacc, mask, first, last):
    H = acts.shape[1]
    m = mask.double()[:, None, :]
    rs = F.conv1d(acts.double(), w.double(), b.double())
    prev = 0.0 if first else outacc.double()
    if last:
        return x.double(), prev + rs * m
    return x.double() + rs[:, :H] * m, prev + rs[:, H:]


def rel_err(a, b):
    return ((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-30)).item()


# ---------------------------------------------------------------------------------------------------------------- the GPU tests' inputs
GATE_TILE_SHAPES = [(2, 192, 77), (2, 128, 300), (1, 256, 77)]                  # ragged 32-column block, 128- and 256-column tile edges
GATE_SPLITK_SHAPES = [(1, 192, 16), (1, 192, 77), (2, 192, 77), (1, 64, 16), (1, 64, 77), (2, 64, 77)]   # H 192: 8 waves, H 64: 4
IN_LAYER_SHAPES = [(2, 192, 77), (1, 192, 16)]
RES_SKIP_SHAPES = [(2, 192, 77, (77, 58)), (1, 128, 200, (163,))]
CHAIN_SHAPE = (2, 192, 77, (77, 58))
CHAIN_LAYERS, CHAIN_GIN = 3, 32


def len_mask(lens, L):
    return (torch.arange(L)[None, :] < torch.tensor(lens)[:, None]).float()


@functools.lru_cache(maxsize=None)
def in_inputs(B, H, L):
    """x, in_layer weight / bias and g_l (reference order), fp32 values: everything nonzero, g_l distinct per item."""
    g = torch.Generator().manual_seed(1000 * H + 10 * L + B)
    x = torch.randn(B, H, L, generator=g)
    w = torch.randn(2 * H, H, K, generator=g) / math.sqrt(H * K)
    b = torch.randn(2 * H, generator=g)
    gl = torch.randn(B, 2 * H, generator=g)
    return x, w, b, gl


@functools.lru_cache(maxsize=None)
def res_skip_inputs(B, H, L, lens):
    """acts, the [2H][H][1] weight / bias, x and outacc before the launch (nonzero in the padded columns too), the mask."""
    g = torch.Generator().manual_seed(77 * H + L)
    acts = torch.randn(B, H, L, generator=g).tanh()
    w = torch.randn(2 * H, H, 1, generator=g) / math.sqrt(H)
    b = torch.randn(2 * H, generator=g)
    x = torch.randn(B, H, L, generator=g)
    outacc = torch.randn(B, H, L, generator=g)
    return acts, w, b, x, outacc, len_mask(lens, L)


@functools.lru_cache(maxsize=None)
def chain_inputs():
    """A 3-layer WN with its cond_layer as a reference-layout state dict (folded `.weight` keys, fp32 values), x (masked, as flow.pre /
    enc_q.pre leave it), g and the ragged mask."""
    B, H, L, lens = CHAIN_SHAPE
    g = torch.Generator().manual_seed(4242)
    sd = {"wn.cond_layer.weight": torch.randn(2 * H * CHAIN_LAYERS, CHAIN_GIN, 1, generator=g) / math.sqrt(CHAIN_GIN),
          "wn.cond_layer.bias": torch.randn(2 * H * CHAIN_LAYERS, generator=g) * 0.1}
    for i in range(CHAIN_LAYERS):
        rows = 2 * H if i < CHAIN_LAYERS - 1 else H
        sd[f"wn.in_layers.{i}.weight"] = torch.randn(2 * H, H, K, generator=g) / math.sqrt(H * K)
        sd[f"wn.in_layers.{i}.bias"] = torch.randn(2 * H, generator=g) * 0.5
        sd[f"wn.res_skip_layers.{i}.weight"] = torch.randn(rows, H, 1, generator=g) / math.sqrt(H)
        sd[f"wn.res_skip_layers.{i}.bias"] = torch.randn(rows, generator=g) * 0.5
    mask = len_mask(lens, L)
    x = torch.randn(B, H, L, generator=g) * mask[:, None, :]
    gvec = torch.randn(B, CHAIN_GIN, generator=g)
    return sd, x, gvec, mask


def chain_layers(sd):
    ins = [(sd[f"wn.in_layers.{i}.weight"], sd[f"wn.in_layers.{i}.bias"]) for i in range(CHAIN_LAYERS)]
    rss = [(sd[f"wn.res_skip_layers.{i}.weight"], sd[f"wn.res_skip_layers.{i}.bias"]) for i in range(CHAIN_LAYERS)]
    return ins, rss
