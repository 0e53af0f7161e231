"""Forced alignment on the device: the reference's own aligner (``SynthesizerTrn.forward``, models.py:960-991) as two handle-free calls.

``neg_cent``       the negative cross-entropy between every latent frame of a recording and every symbol's prior (``bv2_neg_cent``)
``maximum_path``   ``monotonic_align.maximum_path`` over it: frames per symbol, the one-hot path, the path's score (``bv2_maximum_path``)
``align_latent``   both, from a phase-A encode dict and the recording's latent ``z_p``
``kl_path``        the KL between the recording's posterior and the text's prior along a path, per frame and per item (``bv2_kl_path``)
``with_durations`` an encode dict with its durations replaced, ready for ``decode`` — timing transfer is
                   ``align_latent`` -> ``with_durations`` -> ``decode``

Everything runs in kernels/align.hip on the current stream; nothing here computes on the host, and there is no fallback.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional

import torch

from . import lib as L

MAX_SYMBOLS = 4096        # bv2_maximum_path: T
MAX_INTER = 256           # bv2_neg_cent: inter_channels


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _fail(lib, what, rc):
    raise RuntimeError(f"{what} failed ({rc}): {lib.bv2_last_error(None).decode()}")


def check_lengths(x_lengths, y_lengths, T: int, Ty: int) -> None:
    """The aligner's precondition on HOST values (lists, numpy or CPU tensors; device tensors are not read back): 1 <= x_lengths[b] <= T,
    x_lengths[b] <= y_lengths[b] <= Ty.  With more symbols than frames the reference's band is empty and no monotone path exists."""
    on_device = lambda v: isinstance(v, torch.Tensor) and v.is_cuda
    if x_lengths is not None and not on_device(x_lengths):          # what the host knows of x alone
        for b, tx in enumerate(int(v) for v in x_lengths):
            if not 1 <= tx <= T:
                raise ValueError(f"item {b}: x_lengths = {tx} do not fit the [{Ty}, {T}] matrix")
    if x_lengths is None or y_lengths is None or on_device(x_lengths) or on_device(y_lengths):
        return
    xs, ys = [int(v) for v in x_lengths], [int(v) for v in y_lengths]
    if len(xs) != len(ys):
        raise ValueError("x_lengths and y_lengths must have one entry per batch item")
    for b, (tx, ty) in enumerate(zip(xs, ys)):
        if not 1 <= tx <= T or ty > Ty:
            raise ValueError(f"item {b}: x_lengths = {tx} / y_lengths = {ty} do not fit the [{Ty}, {T}] matrix")
        if tx > ty:
            raise ValueError(f"item {b}: {tx} symbols cannot be aligned to {ty} frames (x_lengths must not exceed y_lengths: every symbol "
                             "takes at least one frame)")


@torch.no_grad()
def neg_cent(z_p: torch.Tensor, m_p: torch.Tensor, logs_p: torch.Tensor, x_lengths: Optional[torch.Tensor] = None,
             y_lengths: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``z_p`` [B, inter, Ty], ``m_p`` / ``logs_p`` [B, inter, T] (device fp32) -> [B, Ty, T]; cells outside the lengths are 0."""
    if not z_p.is_cuda:
        raise RuntimeError("bert_vits2_amd.align.neg_cent needs device tensors: there is no CPU fallback")
    lib = L.load()
    dev = z_p.device
    B, D, Ty = z_p.shape
    T = m_p.shape[2]
    if tuple(m_p.shape) != (B, D, T) or tuple(logs_p.shape) != (B, D, T):
        raise ValueError("m_p and logs_p must be [B, inter, T] with z_p's B and inter")
    f32 = lambda t: t.to(dev, torch.float32).contiguous()
    i64 = lambda t: None if t is None else t.to(dev, torch.int64).contiguous()
    z_p, m_p, logs_p, xl, yl = f32(z_p), f32(m_p), f32(logs_p), i64(x_lengths), i64(y_lengths)
    out = torch.empty(B, Ty, T, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        rc = lib.bv2_neg_cent(_stream(), B, D, T, Ty, _ptr(z_p), _ptr(m_p), _ptr(logs_p), _ptr(xl), _ptr(yl), _ptr(out))
    if rc:
        _fail(lib, "bv2_neg_cent", rc)
    return out


@torch.no_grad()
def maximum_path(neg_cent: torch.Tensor, x_lengths, y_lengths, want_attn: bool = False) -> Dict[str, Optional[torch.Tensor]]:
    """``neg_cent`` [B, Ty, T] (device fp32; only read) -> ``durations`` [B, T] int64, ``score`` [B] fp32 and, with ``want_attn``,
    ``attn`` [B, 1, Ty, T].  Lengths given on the host are checked (``check_lengths``); device tensors are taken as they are."""
    if not neg_cent.is_cuda:
        raise RuntimeError("bert_vits2_amd.align.maximum_path needs device tensors: there is no CPU fallback")
    lib = L.load()
    dev = neg_cent.device
    B, Ty, T = neg_cent.shape
    check_lengths(x_lengths, y_lengths, T, Ty)
    as_i64 = lambda t: None if t is None else torch.as_tensor(t).to(dev, torch.int64).contiguous()
    xl, yl = as_i64(x_lengths), as_i64(y_lengths)
    val = neg_cent.to(torch.float32).contiguous()
    nbytes = lib.bv2_maximum_path_workspace_bytes(B, T, Ty)
    if nbytes < 0:
        _fail(lib, "bv2_maximum_path_workspace_bytes", nbytes)
    ws = torch.empty(int(nbytes) // 8, dtype=torch.int64, device=dev)
    dur = torch.empty(B, T, dtype=torch.int64, device=dev)
    score = torch.empty(B, dtype=torch.float32, device=dev)
    attn = torch.empty(B, 1, Ty, T, dtype=torch.float32, device=dev) if want_attn else None
    with torch.cuda.device(dev):
        rc = lib.bv2_maximum_path(_stream(), B, T, Ty, _ptr(val), _ptr(xl), _ptr(yl), _ptr(dur), _ptr(attn), _ptr(score), _ptr(ws),
                                  int(nbytes))
    if rc:
        _fail(lib, "bv2_maximum_path", rc)
    return dict(durations=dur, score=score, attn=attn)


@torch.no_grad()
def align_latent(enc: Dict[str, torch.Tensor], z_p: torch.Tensor, y_lengths, want_attn: bool = False, x_lengths=None) -> Dict:
    """Frames per symbol of a recording whose latent in the prior's space is ``z_p`` [B, inter, Ty], against the text of a phase-A
    encode dict (``m_p``, ``logs_p``, ``x_mask``).  ``x_lengths``: the symbols per item if the caller has them on the host (they are
    then checked against ``y_lengths``); default: counted from ``x_mask`` on the device.  Returns ``durations``, ``y_lengths``, ``score``
    and, with ``want_attn``, ``attn`` and ``neg_cent``."""
    dev = z_p.device
    xl = enc["x_mask"].reshape(z_p.shape[0], -1).sum(1).long() if x_lengths is None else x_lengths
    T, Ty = enc["m_p"].shape[2], z_p.shape[2]
    check_lengths(xl, y_lengths, T, Ty)
    xl_d = torch.as_tensor(xl).to(dev, torch.int64)
    yl_d = torch.as_tensor(y_lengths).to(dev, torch.int64)
    nc = neg_cent(z_p, enc["m_p"], enc["logs_p"], xl_d, yl_d)
    out = maximum_path(nc, xl_d, yl_d, want_attn)
    out["y_lengths"] = yl_d
    out["neg_cent"] = nc if want_attn else None
    return out


@torch.no_grad()
def kl_path(z_p: torch.Tensor, logs_q: torch.Tensor, m_p: torch.Tensor, logs_p: torch.Tensor, durations, x_lengths=None,
            y_lengths=None) -> Dict[str, torch.Tensor]:
    """The KL term of the reference's ``forward()`` (losses.py:45-61) along the path, per frame (``bv2_kl_path``): ``z_p`` / ``logs_q``
    [B, inter, Ty] the recording's latent in the prior's space and its posterior log-std, ``m_p`` / ``logs_p`` [B, inter, T] the text's
    prior, ``durations`` [B, T] frames per symbol (frame j reads the prior of the symbol whose interval holds it: a gather).  Returns
    ``kl_frame`` [B, Ty] (0 at and past ``y_lengths``) and ``kl`` [B], the fixed-order sum of each row; ``kl.sum() / y_lengths.sum()``
    is the reference's ``kl_loss``."""
    if not z_p.is_cuda:
        raise RuntimeError("bert_vits2_amd.align.kl_path needs device tensors: there is no CPU fallback")
    lib = L.load()
    dev = z_p.device
    B, D, Ty = z_p.shape
    T = m_p.shape[2]
    if tuple(logs_q.shape) != (B, D, Ty) or tuple(m_p.shape) != (B, D, T) or tuple(logs_p.shape) != (B, D, T):
        raise ValueError("logs_q must be [B, inter, Ty] and m_p / logs_p [B, inter, T] with z_p's B and inter")
    w = torch.as_tensor(durations)
    if w.numel() != B * T:
        raise ValueError(f"durations must be [B, T] = [{B}, {T}], got {tuple(w.shape)}")
    f32 = lambda t: t.to(dev, torch.float32).contiguous()
    i64 = lambda t: None if t is None else torch.as_tensor(t).to(dev, torch.int64).contiguous()
    z_p, logs_q, m_p, logs_p, w, xl, yl = f32(z_p), f32(logs_q), f32(m_p), f32(logs_p), f32(w.reshape(B, T)), i64(x_lengths), i64(y_lengths)
    out = dict(kl_frame=torch.empty(B, Ty, dtype=torch.float32, device=dev), kl=torch.empty(B, dtype=torch.float32, device=dev))
    with torch.cuda.device(dev):
        rc = lib.bv2_kl_path(_stream(), B, D, T, Ty, _ptr(z_p), _ptr(logs_q), _ptr(m_p), _ptr(logs_p), _ptr(w), _ptr(xl), _ptr(yl),
                             _ptr(out["kl_frame"]), _ptr(out["kl"]))
    if rc:
        _fail(lib, "bv2_kl_path", rc)
    return out


def with_durations(enc: Dict[str, torch.Tensor], durations) -> Dict[str, torch.Tensor]:
    """A copy of a phase-A encode dict with ``w_ceil`` [B, T] replaced by ``durations`` (frames per symbol; any integer or float tensor
    or array of that shape) and ``y_lengths`` by their sums (at least 1, models.py:1057) — what ``decode`` / ``infer_stream`` read.  The other
    entries are shared with ``enc``, not copied."""
    ref = enc["w_ceil"]
    B, T = ref.shape[0], ref.shape[-1]
    d = torch.as_tensor(durations)
    if d.numel() != B * T:
        raise ValueError(f"durations must be [B, T] = [{B}, {T}], got {tuple(d.shape)}")
    if not torch.is_floating_point(d):
        d = d.to(torch.int64)
    if not d.is_cuda and bool((d < 0).any()):             # host values only: a device tensor is not read back
        raise ValueError("durations must not be negative")
    wc = d.to(ref.device, torch.float32).reshape(ref.shape).contiguous()
    out = dict(enc)
    out["w_ceil"] = wc
    out["y_lengths"] = torch.clamp_min(wc.reshape(B, T).sum(1), 1).long()
    return out
