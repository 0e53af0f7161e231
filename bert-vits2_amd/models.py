"""Drop-in ``SynthesizerTrn`` whose ``infer()`` runs on the hand-written gfx950 kernels of ``libbv2.so``.

Mirrors the surface of reference ``models.SynthesizerTrn`` that its callers use
(reference infer.py:84-104, 301-314; train_ms.py:772-784; utils.py:65-120):

* the constructor signature (reference models.py:816-842), unknown ``**kwargs`` swallowed;
* ``.to(device)`` / ``.eval()`` / ``.state_dict()`` / ``.load_state_dict(strict=False)`` with the reference's key
  schema, so reference ``utils.load_checkpoint`` works unchanged;
* ``.infer(x, x_lengths, sid, tone, language, bert, ja_bert, en_bert, noise_scale=.667, length_scale=1,
  noise_scale_w=0.8, max_len=None, sdp_ratio=0, y=None)`` → ``(o, attn, y_mask, (z, z_p, m_p, logs_p))``
  (reference models.py:1026-1074), same shapes/dtypes.  Both speaker branches of models.py:1045-1048 run: ``emb_g(sid)`` with a
  speaker table, ``ref_enc(y)`` (``reference_embedding``) for a model built with ``n_speakers=0``; ``g=`` hands over a speaker
  vector directly (a cached reference voice, a blend of two speakers).

This module is host plumbing only: PyTorch supplies device memory, the current HIP stream and the RNG; every FLOP of
``infer()`` happens inside the C-ABI library.  There is deliberately NO PyTorch/CPU fallback: without a GPU or without
the built library ``infer()`` raises.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import math
import numbers
import weakref
from typing import Dict, NamedTuple, Optional

import torch
from torch import nn

from . import align as _align
from . import hparams as H
from . import lib as L
from .align import with_durations  # noqa: F401  (models.with_durations: an encode dict with its durations replaced)
from .schema import param_shapes


def draw_noise_w(B: int, T: int, device) -> torch.Tensor:
    """Draw #1 of reference infer(), models.py:248-251: ``torch.randn(B, 2, T).to(device=..., dtype=...)`` — taken from the
    global CPU generator even when the model sits on a GPU, then uploaded.  Same call, same stream position: a seeded
    reference run and a seeded run of this shim draw the same SDP noise (RNG contract).  ``device`` None: the draw
    stays on the host (``encode_durations(lean=True)`` uploads it only when the stochastic predictor runs)."""
    return torch.randn(B, 2, T).to(device=device, dtype=torch.float32)


def draw_noise_z(B: int, C: int, Ty: int, device) -> torch.Tensor:
    """Draw #2, models.py:1071: ``torch.randn_like(m_p)`` where ``m_p`` is a TRANSPOSED view ([B,C,T_y] with strides
    (C*T_y, 1, C), models.py:1064-1066) on the model's device.  ``randn_like`` fills in memory order, so only a tensor
    with those strides reproduces the reference's values (plain ``torch.randn(B, C, T_y)`` does not); the
    C ABI takes the strides (``bv2_decode_in.nz_*stride``), so the tensor is handed over as it is."""
    return torch.randn_like(torch.empty(B, Ty, C, device=device, dtype=torch.float32).transpose(1, 2))


class _BlobKind(NamedTuple):
    """One of the model's packed weight blobs: its C entry points, the keys offered to it, where the attached device copy is remembered."""
    c: str                    # the family of C calls: <c>load_tensor, <c>packed_bytes, <c>pack<suffix>, <c>attach<suffix>
    attr: str                 # the attribute that keeps the attached device blob
    prefixes: tuple           # the state-dict keys offered to it (the library itself answers 1 to a key that is not its own)
    suffix: str = ""
    takes_spec: bool = False  # the C calls take spec_channels
    noun: str = "inference weights"
    loader: str = "repack"    # the public method that loads it
    hint: str = ""            # why a checkpoint may not have it


_TRAINING_ONLY = ("is only in TRAINING checkpoints (G_*.pth as utils.save_checkpoint writes them); release checkpoints written by "
                  "compress_model.py are stripped of ")
_INFERENCE = _BlobKind(c="bv2_", suffix="_weights", attr="_blob", prefixes=("",))
_POSTERIOR = _BlobKind(c="bv2_posterior_", attr="_post_blob", prefixes=("enc_q.",), takes_spec=True,
                       noun="posterior encoder", loader="load_posterior",
                       hint="no enc_q.* tensors: the posterior encoder " + _TRAINING_ONLY + "enc_q")
_SDP_FORWARD = _BlobKind(c="bv2_sdp_forward_", attr="_sdpf_blob", prefixes=("sdp.post_", "sdp.flows.1."),
                         noun="forward duration predictor", loader="load_sdp_forward",
                         hint="no sdp.post_* tensors: the posterior side of the stochastic duration predictor " + _TRAINING_ONLY + "it")


def _plain_state_dict(path_or_state_dict) -> Dict[str, torch.Tensor]:
    """A path to a ``G_*.pth``, its dict, or a plain state dict -> a plain state dict without DDP's ``module.`` prefix."""
    sd = path_or_state_dict
    if isinstance(sd, (str, bytes)) or hasattr(sd, "__fspath__"):
        sd = torch.load(sd, map_location="cpu")
    if isinstance(sd, dict) and "model" in sd and isinstance(sd["model"], dict):
        sd = sd["model"]
    return {(k[7:] if k.startswith("module.") else k): v for k, v in sd.items()}


NOISE_W, NOISE_Z, NOISE_Q = 0, 1, 2     # ``which`` of the seeded generator (csrc/kernels/rng.h): the SDP draw, the prior draw, the posterior draw
NOISE_E = 3                             # e_q of the duration likelihood (``duration_nll``); computed in its kernel only, ``seeded_noise`` offers 0-2


def item_seeds(seeds, B: int, device) -> Optional[torch.Tensor]:
    """``seeds`` as ``infer`` takes it -> int64 ``[B]`` on ``device`` (None stays None).  An int is applied to every item; a sequence
    of B ints or an int64 tensor ``[B]`` gives one seed per utterance.  Any int64 is a seed (the generator reads its bit pattern)."""
    if seeds is None:
        return None
    if isinstance(seeds, numbers.Integral) and not isinstance(seeds, bool):
        seeds = [int(seeds)] * B
    if not isinstance(seeds, torch.Tensor):
        try:
            seeds = torch.tensor([int(v) for v in seeds], dtype=torch.int64)
        except (TypeError, ValueError, RuntimeError, OverflowError) as e:
            raise ValueError(f"seeds must be an int, B = {B} ints in the int64 range or an int64 tensor [B]") from e
    if seeds.dtype != torch.int64 or tuple(seeds.shape) != (B,):
        raise ValueError(f"seeds must be an int, B = {B} ints or an int64 tensor [B], got {seeds.dtype} {tuple(seeds.shape)}")
    return seeds.detach().to(device).contiguous()


def seeded_noise(seeds, which: int, rows: int, T: int, lengths=None, device=None, transposed: bool = False) -> torch.Tensor:
    """The seeded generator's N(0,1) values as a tensor ``[B, rows, T]`` (``bv2_seeded_noise``): element (b, r, t) is the value the
    kernels compute in place for utterance seed ``seeds[b]``, draw ``which`` (``NOISE_W`` / ``NOISE_Z`` / ``NOISE_Q``), row r, frame t —
    bit for bit, so ``infer(noise_w=seeded_noise(s, 0, 2, T), noise_z=seeded_noise(s, 1, C, Ty, lengths=y_lengths))`` is
    ``infer(seeds=s)``.  ``seeds``: a sequence of ints or an int64 tensor ``[B]``; ``lengths`` [B]: frames at or past it are 0;
    ``transposed``: the tensor has the reference's strides ``(T * rows, 1, rows)`` (``draw_noise_z``)."""
    if isinstance(seeds, numbers.Integral):
        seeds = [int(seeds)]
    if device is None:
        device = seeds.device if isinstance(seeds, torch.Tensor) and seeds.is_cuda else torch.device("cuda")
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("bert_vits2_amd.models.seeded_noise needs a GPU: no CPU fallback exists by design")
    B = int(seeds.shape[0]) if isinstance(seeds, torch.Tensor) else len(seeds)
    sd = item_seeds(seeds, B, device)
    rows, T = int(rows), int(T)
    if B < 1 or rows < 1 or T < 1:
        raise ValueError("seeded_noise needs B, rows and T of at least 1")
    ln = None if lengths is None else torch.as_tensor(lengths).to(device, torch.int64).reshape(B).contiguous()
    out = torch.empty(B, T, rows, dtype=torch.float32, device=device).transpose(1, 2) if transposed else \
        torch.empty(B, rows, T, dtype=torch.float32, device=device)
    lib = L.load()
    with torch.cuda.device(device):
        rc = lib.bv2_seeded_noise(C.c_void_p(torch.cuda.current_stream().cuda_stream), _ptr(sd), B, int(which), rows, T, _ptr(ln),
                                  _ptr(out), out.stride(0), out.stride(1), out.stride(2))
    if rc:
        raise RuntimeError(f"bv2_seeded_noise failed ({rc}): {lib.bv2_last_error(None).decode()}")
    return out


def item_control(name: str, value, B: int, device):
    """One synthesis control (``sdp_ratio``, ``noise_scale``, ``noise_scale_w``, ``length_scale``) as ``infer`` takes it.  A Python
    number or a 0-d tensor -> ``(float, None)``: the scalar path.  A tensor of B elements shaped ``[B]``, ``[B,1]`` or ``[B,1,1]``
    (the shapes the reference's ``infer`` broadcasts) -> ``(None, fp32 [B] on device)``: one value per utterance
    (``bv2_item_controls``; ``device`` None keeps the tensor where it is).  Any other shape raises ValueError naming the control."""
    if not isinstance(value, torch.Tensor):
        if isinstance(value, numbers.Real):
            return float(value), None
        try:
            value = torch.as_tensor(value)
        except (TypeError, ValueError, RuntimeError) as e:
            raise ValueError(f"{name} must be a number or a tensor of B = {B} values") from e
    if value.dim() == 0:
        return float(value), None
    if tuple(value.shape) not in ((B,), (B, 1), (B, 1, 1)):
        raise ValueError(f"{name} must be a number or a tensor shaped [B], [B,1] or [B,1,1] with B = {B}, got {tuple(value.shape)}")
    return None, value.detach().to(device=device or value.device, dtype=torch.float32).reshape(B).contiguous()


def _control_buffer(values) -> torch.Tensor:
    """A zeroed [4, B] fp32 control buffer, on the host when every per-item value is there (then one upload moves it)."""
    t = [v for v in values if v is not None]
    host = all(v.device.type == "cpu" for v in t)
    return torch.zeros(4, t[0].shape[0], dtype=torch.float32, device="cpu" if host else t[0].device)


def _controls_ptr(ctl: Optional[torch.Tensor], rows):
    """bv2_item_controls over the rows of a [4, B] fp32 control buffer (noise_scale_w, sdp_ratio, length_scale, noise_scale);
    ``rows`` names the members that are set, the others stay null."""
    if ctl is None:
        return None
    ic = L.ItemControls()
    ic.struct_bytes = C.sizeof(L.ItemControls)
    for r, name in enumerate(("noise_scale_w", "sdp_ratio", "length_scale", "noise_scale")):
        if r in rows:
            setattr(ic, name, ctl[r].data_ptr())
    return C.byref(ic)


class _Node(nn.Module):
    """A bare namespace module: only there so that parameters carry the reference's dotted names."""

    def forward(self, *a, **k):  # pragma: no cover
        raise NotImplementedError("bert_vits2_amd exposes SynthesizerTrn.infer() only; sub-modules are parameter holders")


def _substitute_durations(enc, w_ceil, items, B: int, T: int, dev) -> None:
    """``infer(w_ceil=...)`` / ``infer_stream(w_ceil=...)``: the given durations take the place of phase A's in ``enc`` (in place), with
    ``y_lengths`` = their sums (at least 1, models.py:1057).  ``items`` [B] bool: only the marked items, the others keep their own."""
    wc = w_ceil.to(dev, torch.float32).reshape(B, T).contiguous()
    if items is not None:
        keep = torch.as_tensor(items).to(dev, torch.bool).reshape(B, 1)
        wc = torch.where(keep, wc, enc["w_ceil"].reshape(B, T))
    enc["w_ceil"] = wc
    enc["y_lengths"] = torch.clamp_min(wc.sum(1), 1).long()


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


class _LastEncode(dict):
    """``SynthesizerTrn.last_encode``: what phase A of the last ``infer`` / ``infer_stream`` returned.  They ask for the lean form
    (``encode_durations(lean=True)``), which at ``sdp_ratio`` 0 carries no ``logw_sdp`` and at 1 no ``logw_dp``; a reader that indexes the
    missing one gets it computed on first access by that predictor's single-stage call (``stage_sdp`` / ``stage_dp``) on the kept encoder
    output — parity tests and debugging, off the hot path.  It is not among ``keys()`` until then."""

    def __init__(self, enc, model, noise_w, noise_scale_w, seeds=None):
        super().__init__(enc)
        self._model, self._noise_w, self._noise_scale_w, self._seeds = weakref.ref(model), noise_w, noise_scale_w, seeds

    def __missing__(self, key):
        m = self._model()
        if key not in ("logw_sdp", "logw_dp") or m is None:
            raise KeyError(key)
        if key == "logw_dp":
            v = m.stage_dp(self["x"], self["x_mask"], self["g"])[:, 0]
        else:
            B = self["x"].shape[0]
            scale, per_item = item_control("noise_scale_w", self._noise_scale_w, B, m.device)
            nw = self._noise_w if self._seeds is None else seeded_noise(self._seeds, NOISE_W, 2, self["x"].shape[2], device=m.device)
            zin = nw.to(m.device, torch.float32) * (scale if per_item is None else per_item.reshape(B, 1, 1))
            v = m.stage_sdp(self["x"], self["x_mask"], zin, self["g"])[:, 0]
        self[key] = v
        return v


class SynthesisStream:
    """What ``SynthesizerTrn.infer_stream`` returns: an iterator of ``(start_sample, audio[B, n])``.  Phase A, the one host sync and the
    flow have run when it exists; every ``next()`` enqueues one windowed Generator decode (``bv2_stream_chunk``) on the current stream and
    hands back a fresh tensor.  The chunks tile ``[0, total_samples)`` exactly and in order; rows are zero past an item's end.

    ``y_lengths`` [B] (device, frames; ``y_lengths_host`` is the list read at the host sync), ``Ty``, ``total_samples`` (= frames fed to the Generator x product of the upsample rates), ``halo``
    (frames a window carries on each side, ``hparams.generator_halo``) and ``aux`` (``attn``, ``y_mask``, ``z``, ``z_p``, ``m_p``,
    ``logs_p`` as ``infer`` returns them) are there from the start.  The stream owns its workspace, so other ``infer`` calls of the same
    model may run between two chunks; call ``next()`` on the stream ``infer_stream`` ran on (or one ordered behind it)."""

    def __init__(self, model, enc, ws, Ty, frames, bounds, window_frames, exact_lengths, as_pcm16, pcm_gain, aux, output_rate=None):
        self._model, self._enc, self._ws = model, enc, ws
        self.y_lengths, self.Ty, self.aux = enc["y_lengths"], int(Ty), aux
        self.halo = H.generator_halo(model.hp)
        self._U = model.hp.total_upsample
        self.total_samples = int(frames) * self._U
        self._frames, self._bounds, self._next = int(frames), list(bounds), 0
        self._window, self._exact, self._pcm, self._gain = int(window_frames), int(bool(exact_lengths)), bool(as_pcm16), float(pcm_gain)
        self.max_chunk_samples = self._window * self._U
        self._rs = None
        if output_rate is not None and int(output_rate) != int(model.hp.sampling_rate):
            self._init_resampler(int(model.hp.sampling_rate), int(output_rate))

    def _init_resampler(self, rate_in, rate_out):
        """With ``output_rate`` the chunks leave at that rate: a rolling fp32 device buffer holds the tail of the model-rate audio that
        later outputs still read (at most ``2K + M / L + 2`` samples) in front of the new chunk; after the chunk that ends at model-rate
        sample E the outputs ``[done, min(bv2_resample_ready(E), N_total))`` are emitted (everything up to ``N_total`` at the last one).
        An output's sum does not depend on the range it is emitted in (include/bv2.h), so the pieces are the one-shot result's."""
        from . import audio
        Lr, M, K = audio.resample_plan(rate_in, rate_out)
        dev, B = self._ws.device, self.y_lengths.shape[0]
        total_in = self.total_samples
        # item b is its own y_lengths[b] * U samples with exact_lengths, else everything the Generator wrote for it
        lens = self.y_lengths.to(torch.int64) * self._U if self._exact else torch.full((B,), total_in, dtype=torch.int64, device=dev)
        self._rs = dict(rate_in=rate_in, rate_out=rate_out, L=Lr, M=M, K=K, cfg=audio.resample_config(rate_in, rate_out), lens=lens,
                        out_lens=torch.empty(B, dtype=torch.int64, device=dev), total_in=total_in, tail=None, start=0, done=0)
        self.total_samples = audio.resample_length(rate_in, rate_out, total_in)
        self.max_chunk_samples = -((-(self._window * self._U + 2 * K + 1) * Lr) // M) + 1

    def __iter__(self):
        return self

    def __len__(self):
        return len(self._bounds)

    def _chunk(self, t0, t1, out, bstride, pcm):
        """One ``bv2_stream_chunk`` on the current stream: samples [t0 * U, t1 * U) to ``out`` (a tensor whose first element is sample
        t0 * U of item 0, rows ``bstride`` apart)."""
        m, B = self._model, self.y_lengths.shape[0]
        a = L.StreamChunkArgs()
        a.struct_bytes = C.sizeof(L.StreamChunkArgs)
        a.B, a.Ty, a.t0, a.t1 = B, self.Ty, t0, t1
        a.y_lengths, a.exact_lengths = self.y_lengths.data_ptr(), self._exact
        if pcm:
            a.dst16, a.dst16_bstride, a.pcm_gain = out.data_ptr(), bstride, self._gain
        else:
            a.dst, a.dst_bstride = out.data_ptr(), bstride
        a.window_frames, a.max_len = self._window, self._frames
        with torch.cuda.device(self._ws.device):
            m._check(m._lib.bv2_stream_chunk(m._handle, C.c_void_p(torch.cuda.current_stream().cuda_stream), C.byref(a),
                                             C.c_void_p(self._ws.data_ptr()), self._ws.numel()), "bv2_stream_chunk")

    def __next__(self):
        if self._rs is not None:
            return self._next_resampled()
        if self._next >= len(self._bounds):
            raise StopIteration
        t0, t1 = self._bounds[self._next]
        B, n = self.y_lengths.shape[0], (t1 - t0) * self._U
        out = torch.empty(B, n, dtype=torch.int16 if self._pcm else torch.float32, device=self._ws.device)
        self._chunk(t0, t1, out, n, self._pcm)
        self._next += 1
        return t0 * self._U, out

    def _next_resampled(self):
        from . import audio
        rs, m, dev, B = self._rs, self._model, self._ws.device, self.y_lengths.shape[0]
        while self._next < len(self._bounds):
            t0, t1 = self._bounds[self._next]
            last = self._next == len(self._bounds) - 1
            self._next += 1
            n, E = (t1 - t0) * self._U, t1 * self._U
            keep = 0 if rs["tail"] is None else rs["tail"].shape[1]
            buf = torch.empty(B, keep + n, dtype=torch.float32, device=dev)       # samples [rs["start"], E) of every item
            if keep:
                buf[:, :keep].copy_(rs["tail"])
            self._chunk(t0, t1, buf[:, keep:], keep + n, False)
            lib = m._lib
            ready = self.total_samples if last else min(int(lib.bv2_resample_ready(C.byref(rs["cfg"]), E)), self.total_samples)
            done = rs["done"]
            if ready <= done:                                                      # nothing has its whole support yet: keep everything
                rs["tail"] = buf
                continue
            out = audio.resample_range(buf, rs["start"], rs["lens"], rs["rate_in"], rs["rate_out"], done, ready, None, rs["out_lens"])
            first = max(rs["start"], (ready * rs["M"]) // rs["L"] - rs["K"], 0)     # the next range's lower edge
            rs["tail"], rs["start"], rs["done"] = (buf[:, first - rs["start"]:] if first < E else None), min(first, E), ready
            if self._pcm:                                                          # fixed gain on the resampled samples; the clamp takes the filter's overshoot
                pcm = torch.empty(B, ready - done, dtype=torch.int16, device=dev)
                with torch.cuda.device(dev):
                    rc = lib.bv2_emit(C.c_void_p(torch.cuda.current_stream().cuda_stream), C.c_void_p(out.data_ptr()), ready - done, 0,
                                      C.c_void_p(rs["out_lens"].data_ptr()), 1, done, B, ready - done, None, C.c_void_p(pcm.data_ptr()),
                                      ready - done, self._gain)
                if rc:
                    raise RuntimeError(f"bv2_emit failed ({rc}): {lib.bv2_last_error(None).decode()}")
                out = pcm
            return done, out
        raise StopIteration


class SynthesizerTrn(nn.Module):
    """Synthesizer (inference path) — see module docstring."""

    def __init__(self, n_vocab, spec_channels, segment_size, inter_channels, hidden_channels, filter_channels, n_heads,
                 n_layers, kernel_size, p_dropout, resblock, resblock_kernel_sizes, resblock_dilation_sizes,
                 upsample_rates, upsample_initial_channel, upsample_kernel_sizes, n_speakers=256, gin_channels=256,
                 use_sdp=True, n_flow_layer=4, n_layers_trans_flow=4, flow_share_parameter=False,
                 use_transformer_flow=True, **kwargs):
        super().__init__()
        self.hp = H.from_ctor(
            n_vocab, spec_channels, segment_size, inter_channels=inter_channels, hidden_channels=hidden_channels,
            filter_channels=filter_channels, n_heads=n_heads, n_layers=n_layers, kernel_size=kernel_size,
            p_dropout=p_dropout, resblock=resblock, resblock_kernel_sizes=list(resblock_kernel_sizes),
            resblock_dilation_sizes=[list(d) for d in resblock_dilation_sizes], upsample_rates=list(upsample_rates),
            upsample_initial_channel=upsample_initial_channel, upsample_kernel_sizes=list(upsample_kernel_sizes),
            n_speakers=n_speakers, gin_channels=gin_channels, use_sdp=use_sdp, n_flow_layer=n_flow_layer,
            n_layers_trans_flow=n_layers_trans_flow, flow_share_parameter=flow_share_parameter,
            use_transformer_flow=use_transformer_flow)
        self.hp.validate()
        # attributes the reference exposes and callers read
        self.n_vocab, self.spec_channels, self.segment_size = n_vocab, spec_channels, segment_size
        self.inter_channels, self.hidden_channels, self.filter_channels = inter_channels, hidden_channels, filter_channels
        self.n_heads, self.n_layers, self.kernel_size, self.p_dropout = n_heads, n_layers, kernel_size, p_dropout
        self.n_speakers, self.gin_channels = n_speakers, gin_channels
        self.use_sdp = use_sdp
        for key, shape in param_shapes(self.hp).items():
            # placeholders until a checkpoint is loaded: LayerNorm gamma / weight_norm g at 1 (the reference's own defaults,
            # modules.py:22-23), everything else 0.  infer() refuses to run on them (see repack).
            leaf = key.rsplit(".", 1)[-1]
            init = torch.ones if leaf in ("gamma", "weight_g") else torch.zeros
            self._register(key, init(shape, dtype=torch.float32))
        self._params_loaded = False
        self._lib = None
        self._handle = C.c_void_p()
        self._blob: Optional[torch.Tensor] = None
        self._ws: Optional[torch.Tensor] = None
        self._taps: Dict[str, torch.Tensor] = {}
        self.generator_dtype = torch.float32
        self.flow_dtype = torch.float32
        self._graphs_on = False
        self._graphs_static = False
        self._ty_bucket = 32
        self.graph_stats = dict(captures=0, replays=0)
        self._graphs: Dict[tuple, dict] = {}
        self._cap_stream = None
        self._options: Dict[str, int] = {}
        self._stft_params = None           # audio.StftParams of reference_embedding_from_wav (None: what the hyper-parameters imply)
        self.ref_encode_calls = 0          # bv2_ref_encode calls made through reference_embedding (serving encodes a shared reference once)

    # ------------------------------------------------------------------ parameter tree
    def _register(self, key: str, value: torch.Tensor) -> None:
        node = self
        parts = key.split(".")
        for p in parts[:-1]:
            if p not in node._modules:
                node.add_module(p, _Node())
            node = node._modules[p]
        node.register_parameter(parts[-1], nn.Parameter(value, requires_grad=False))

    def _invalidate_weights(self) -> None:
        """The packed device blob no longer matches the parameters (or is about to move): forget it everywhere — captured
        graphs baked its address in, and the C handle must not keep pointing at memory torch may free."""
        if getattr(self, "_graphs", None):
            self._drop_graphs()
        if getattr(self, "_lib", None) is not None and getattr(self, "_handle", None):
            self._lib.bv2_detach_weights(self._handle)
        self._blob = None

    def load_state_dict(self, state_dict, strict: bool = True, **kw):
        self._invalidate_weights()
        self._params_loaded = True
        if not strict:
            # the reference loads with strict=False and tolerates training-only keys (enc_q.*, sdp.post_*)
            own = set(k for k, _ in self.named_parameters())
            state_dict = {k: v for k, v in state_dict.items() if k in own}
        return super().load_state_dict(state_dict, strict=strict, **kw)

    def _apply(self, fn, *a, **k):
        if hasattr(self, "_blob"):
            self._invalidate_weights()
        self._ws = None
        return super()._apply(fn, *a, **k)

    def forward(self, *a, **k):
        raise NotImplementedError("training forward() is out of scope; this class accelerates infer() only")

    # ------------------------------------------------------------------ native handle / weights
    @property
    def device(self) -> torch.device:
        # a rank that only received the packed blob (sharding.distribute_weights) runs where the blob lives
        if self._blob is not None:
            return self._blob.device
        return next(self.parameters()).device

    def _ensure_handle(self):
        if self._lib is None:
            self._lib = L.load()
            cfg = L.make_config(self.hp)
            rc = self._lib.bv2_create(C.byref(cfg), C.byref(self._handle))
            if rc:
                raise RuntimeError("bv2_create failed: " + self._lib.bv2_last_error(None).decode())
        return self._lib

    def _check(self, rc: int, what: str):
        if rc:
            raise RuntimeError(f"{what} failed ({rc}): {self._lib.bv2_last_error(self._handle).decode()}")

    def __del__(self):
        try:
            self._drop_graphs()
            if self._lib is not None and self._handle:
                self._lib.bv2_destroy(self._handle)
        except Exception:
            pass

    # ---- the packed weight blobs (_BlobKind): host tensors -> packed host blob; device blob -> attached and remembered
    def _pack_kind(self, kind: _BlobKind, tensors) -> torch.Tensor:
        lib = self._ensure_handle()
        spec = (int(self.hp.spec_channels),) if kind.takes_spec else ()
        n = getattr(lib, kind.c + "packed_bytes")(self._handle, *spec)
        if n < 0:
            self._check(-1, kind.c + "packed_bytes")
        for key, v in tensors:
            if not key.startswith(kind.prefixes):
                continue
            t = v.detach().to("cpu", torch.float32).contiguous()
            shape = (C.c_int64 * t.dim())(*t.shape)
            rc = getattr(lib, kind.c + "load_tensor")(self._handle, key.encode(), C.c_void_p(t.data_ptr()), shape, t.dim(), L.F32)
            if rc < 0:                         # rc == 1: a key this blob ignores (the inference blob: sdp.flows.1.*)
                self._check(rc, kind.c + "load_tensor(" + key + ")")
        blob = torch.empty(n, dtype=torch.uint8)
        pack = kind.c + "pack" + kind.suffix
        self._check(getattr(lib, pack)(self._handle, *spec, C.c_void_p(blob.data_ptr()), n), pack)
        return blob

    def _attach_kind(self, kind: _BlobKind, dev_blob: torch.Tensor) -> None:
        spec = (int(self.hp.spec_channels),) if kind.takes_spec else ()
        attach = kind.c + "attach" + kind.suffix
        self._check(getattr(self._ensure_handle(), attach)(self._handle, *spec, C.c_void_p(dev_blob.data_ptr()), dev_blob.numel()), attach)
        setattr(self, kind.attr, dev_blob)

    def _load_kind(self, kind: _BlobKind, host_blob: torch.Tensor) -> None:
        dev = self.device
        if dev.type != "cuda":
            raise RuntimeError(f"{kind.loader} needs the model on a GPU (model.to('cuda')); there is no CPU fallback")
        with torch.cuda.device(dev):
            self._attach_kind(kind, host_blob.to(dev))

    def _need_kind(self, kind: _BlobKind, what: str) -> None:
        blob = getattr(self, kind.attr, None)
        if blob is None:
            raise RuntimeError(f"{what}: the {kind.noun} is not loaded ({kind.loader}(checkpoint)); " + kind.hint)
        if blob.device != self.device:
            raise RuntimeError(f"{what}: the model moved to another device after {kind.loader}(); load it again")

    def pack_host_blob(self) -> torch.Tensor:
        """Fold weight-norm / repack every tensor into the library's blob (host, uint8).  CPU-only: usable without a GPU."""
        return self._pack_kind(_INFERENCE, self.named_parameters())

    def attach_blob(self, dev_blob: torch.Tensor) -> None:
        """Use an already packed blob resident on this GPU (e.g. received through an RCCL broadcast)."""
        assert dev_blob.is_cuda and dev_blob.dtype == torch.uint8 and dev_blob.is_contiguous()
        self._drop_graphs()
        self._attach_kind(_INFERENCE, dev_blob)

    def repack(self) -> None:
        """(Re)build the packed device weights from the current parameters (call after editing parameters in place)."""
        dev = self.device
        if dev.type != "cuda":
            raise RuntimeError("bert_vits2_amd.SynthesizerTrn.infer needs the model on a GPU (model.to('cuda')); "
                               "there is no CPU fallback")
        if not self._params_loaded:
            raise RuntimeError("no weights: this SynthesizerTrn never saw load_state_dict() / load_checkpoint() (a rank that only "
                               "received the packed blob must attach_blob() again after .to(); it has no parameters to repack)")
        with torch.cuda.device(dev):
            self.attach_blob(self.pack_host_blob().to(dev))

    def set_generator_dtype(self, dtype) -> None:
        """Arithmetic of the Generator (``dec``): ``torch.float32`` (default, exact fp32 MFMA) or ``torch.bfloat16``
        (bf16 weights + channels-last bf16 activations, fp32 accumulate — BASELINE config 3; the reference's counterpart
        is running ``dec`` under ``torch.autocast(bfloat16)``).  Encoder, durations and flow stay fp32 either way."""
        lib = self._ensure_handle()
        code = {torch.float32: L.F32, "fp32": L.F32, "f32": L.F32, torch.bfloat16: L.BF16, "bf16": L.BF16}.get(dtype)
        if code is None:
            raise ValueError("generator dtype must be torch.float32 or torch.bfloat16")
        self._check(lib.bv2_set_generator_dtype(self._handle, code), "bv2_set_generator_dtype")
        self._drop_graphs()
        self.generator_dtype = torch.bfloat16 if code == L.BF16 else torch.float32

    def set_flow_dtype(self, dtype) -> None:
        """Arithmetic of the transformer flow's Encoder convolutions (fused q/k/v, conv_o, FFN): ``torch.float32``
        (default) or ``torch.float16`` (fp16 weights / conv inputs / FFN hidden, fp32 accumulate — BASELINE config 5
        "fp16 flow + fp32 spline"; the reference's counterpart is ``flow`` under ``torch.autocast(float16)``); the attention
        core's QK^T / PV products take fp16 operands too.  LayerNorm, softmax, the residual stream and everything before the
        flow stay fp32: durations are unchanged."""
        lib = self._ensure_handle()
        code = {torch.float32: L.F32, "fp32": L.F32, "f32": L.F32, torch.float16: L.F16, "fp16": L.F16, "f16": L.F16}.get(dtype)
        if code is None:
            raise ValueError("flow dtype must be torch.float32 or torch.float16")
        self._check(lib.bv2_set_flow_dtype(self._handle, code), "bv2_set_flow_dtype")
        self._drop_graphs()
        self.flow_dtype = torch.float16 if code == L.F16 else torch.float32

    @contextlib.contextmanager
    def _seeded(self, seeds: Optional[torch.Tensor]):
        """The library calls inside draw from ``seeds`` (int64 [B] on the device, ``bv2_set_noise_seeds``); None: nothing changes."""
        if seeds is None:
            yield
            return
        self._check(self._lib.bv2_set_noise_seeds(self._handle, _ptr(seeds), int(seeds.shape[0])), "bv2_set_noise_seeds")
        try:
            yield
        finally:
            self._lib.bv2_set_noise_seeds(self._handle, None, 0)

    def _workspace(self, B: int, T: int, Ty: int) -> torch.Tensor:
        n = self._lib.bv2_workspace_bytes(self._handle, B, T, Ty)
        if n < 0:
            raise RuntimeError("bv2_workspace_bytes failed")
        if self._ws is None or self._ws.numel() < n or self._ws.device != self.device:
            self._drop_graphs()                    # captured graphs bake in the workspace address
            self._ws = torch.empty(int(n * 1.25), dtype=torch.uint8, device=self.device)
        return self._ws

    # ------------------------------------------------------------------ hipGraph replay of the two phases
    def enable_graphs(self, on: bool = True, static_io: bool = False, ty_bucket: int = 32) -> None:
        """Record each phase once per shape as a hipGraph (``bv2_graph_capture_*``) and replay it on later calls: one
        ``hipGraphLaunch`` per phase instead of ~230 kernel launches.  Default: inputs are copied into buffers the graph owns and
        outputs are returned as fresh tensors, so the call behaves exactly like the eager one.

        ``ty_bucket`` (frames): ``T_y = max(y_lengths)`` is data-dependent (reference commons.py:119-123, models.py:1058), so with real
        durations nearly every batch has a T_y of its own.  Phase B is therefore recorded once per BUCKET — T_y rounded up to a multiple of
        ``ty_bucket`` — and replayed for every T_y inside it: the flow masks frames past ``y_lengths`` as in any ragged batch, the Generator
        treats everything past the batch's longest utterance as zero padding (``bv2_decode_in.exact_lengths`` 2, or 1 with
        ``exact_lengths=True``), and the returned tensors are views cut back to the true T_y.  The results are those of the eager call up to
        fp32 summation order (a bucket may pick another split-K factor); ``ty_bucket=1`` keys graphs on the exact T_y (bit-identical to
        eager, one capture per distinct T_y).  ``graph_stats`` counts captures and replays.

        ``static_io=True`` (serving loops): no staging copies — a graph is recorded reading the caller's input tensors IN PLACE
        (when a tensor with another address shows up the shape's graph is re-recorded ONCE with input buffers of its own and the
        inputs are copied in from then on; up to 16 shapes are cached) and the returned tensors are the graph's own output buffers, valid until the next call with the same shapes.  Only the two noise draws still move:
        the CPU draw of models.py:248-251 is uploaded into the graph's buffer, the device draw of :1071 is made in place."""
        self._graphs_on = bool(on)
        self._graphs_static = bool(on and static_io)
        self._ty_bucket = max(1, int(ty_bucket))
        self.graph_stats = dict(captures=0, replays=0)
        self._drop_graphs()

    def _drop_graphs(self) -> None:
        graphs, self._graphs = getattr(self, "_graphs", {}), {}
        for g in graphs.values():
            if self._lib is not None and g.get("graph"):
                self._lib.bv2_graph_destroy(g["graph"])

    def _capture(self, fn, *args):
        """Run one capture call on a dedicated non-default stream (the legacy default stream cannot be captured)."""
        dev = self.device
        if self._cap_stream is None or self._cap_stream.device != dev:
            self._cap_stream = torch.cuda.Stream(device=dev)
        torch.cuda.current_stream(dev).synchronize()      # buffers the graph will touch are idle while it is recorded
        g = C.c_void_p()
        self._check(fn(self._handle, C.c_void_p(self._cap_stream.cuda_stream), *args, C.byref(g)), fn.__name__)
        return g

    def _graph_entry(self, key, build, ptrs=()):
        """Cached graph for ``key`` (shapes + scalars).  ``ptrs``: addresses of the tensors a static_io graph reads in place.  A
        graph recorded on other addresses is NOT re-recorded per call: the first pointer miss rebuilds the entry ONCE with input
        buffers the graph owns (``build(own_inputs=True)``) and from then on inputs are copied in — a caller that re-materialises
        its inputs every call (CPU tensors, the ``w_ceil=`` override, fresh uploads) costs one copy per call, not one capture."""
        ent = self._graphs.get(key)
        if ent is not None and not ent["own_inputs"] and ent["ptrs"] != ptrs:
            self._lib.bv2_graph_destroy(self._graphs.pop(key)["graph"])
            ent = None
            own = True
        else:
            own = not self._graphs_static
        if ent is None:
            if len(self._graphs) >= 16:                   # bounded cache: drop the least recently used shape
                old = next(iter(self._graphs))
                self._lib.bv2_graph_destroy(self._graphs.pop(old)["graph"])
            ent = build(own)
            ent["own_inputs"], ent["ptrs"] = own, ptrs
            self._graphs[key] = ent
            self.graph_stats["captures"] += 1
        else:
            self._graphs[key] = self._graphs.pop(key)     # most recently used last
            self.graph_stats["replays"] += 1
        return ent

    def set_tap(self, name: Optional[str], tensor: Optional[torch.Tensor] = None) -> None:
        """Debug: copy a named intermediate into ``tensor`` (fp32, CUDA) during the next calls."""
        lib = self._ensure_handle()
        if name is None:
            self._taps.clear()
            lib.bv2_set_tap(self._handle, None, None, 0)
            return
        if tensor is None:
            self._taps.pop(name, None)
            lib.bv2_set_tap(self._handle, name.encode(), None, 0)
            return
        self._taps[name] = tensor
        lib.bv2_set_tap(self._handle, name.encode(), C.c_void_p(tensor.data_ptr()), tensor.numel())

    # ------------------------------------------------------------------ speaker vectors
    def _speaker_vector(self, g, B: int) -> torch.Tensor:
        """A caller's ``g`` as fp32 [B, gin] on the model's device; accepts [B, gin] and the reference's [B, gin, 1]."""
        gin = self.hp.gin_channels
        if not isinstance(g, torch.Tensor) or tuple(g.shape) not in ((B, gin), (B, gin, 1)):
            raise ValueError(f"g must be a tensor shaped [B, gin] or [B, gin, 1] with B = {B}, gin = {gin}, got "
                             f"{tuple(g.shape) if isinstance(g, torch.Tensor) else type(g).__name__}")
        return g.detach().to(self.device, torch.float32).reshape(B, gin).contiguous()

    @torch.no_grad()
    def reference_embedding(self, y: torch.Tensor, y_lengths: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``ref_enc(y.transpose(1, 2))`` of reference models.py:1047-1048 -> g [B, gin]: the voice of a reference recording, for a model
        built with ``n_speakers=0``.  ``y`` is the linear spectrogram [B, spec_channels, L] as the reference's ``infer`` takes it (any
        strides: it is read in place).  ``y_lengths`` [B] makes a padded batch exact: every layer treats item b's frames past its own
        length as zero padding and its GRU stops after its last step, so each row is bit for bit what that reference gives alone
        (``None``: all L frames of every item count, the reference's own semantics).  Eight launches, outside the graphs (the shape
        depends on L); compute it once per voice and pass it to ``infer(g=...)``."""
        if self.hp.n_speakers != 0:
            raise RuntimeError("reference_embedding needs a model built with n_speakers=0 (this one has a speaker table: emb_g)")
        if self._blob is None:
            self.repack()
        dev = self.device
        if y.dim() != 3 or y.shape[1] != self.hp.spec_channels or y.shape[2] < 1:
            raise ValueError(f"y must be [B, spec_channels = {self.hp.spec_channels}, L >= 1], got {tuple(y.shape)}")
        y = y.detach().to(dev, torch.float32)
        B, _, Lf = y.shape
        yl = None
        if y_lengths is not None:
            yl = torch.as_tensor(y_lengths).to(dev, torch.int64).reshape(-1).contiguous()
            if yl.shape != (B,):
                raise ValueError("y_lengths must be [B]")
        n = self._lib.bv2_ref_workspace_bytes(self._handle, B, Lf)
        if n < 0:
            raise RuntimeError("bv2_ref_workspace_bytes failed")
        ws = torch.empty(n, dtype=torch.uint8, device=dev)      # sized by L: not the phases' workspace (captured graphs bake that one in)
        g = torch.empty(B, self.hp.gin_channels, dtype=torch.float32, device=dev)
        strides = (C.c_int64 * 3)(*y.stride())
        with torch.cuda.device(dev):
            stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            self._check(self._lib.bv2_ref_encode(self._handle, stream, _ptr(y), strides, _ptr(yl), B, Lf, _ptr(g),
                                                 C.c_void_p(ws.data_ptr()), ws.numel()), "bv2_ref_encode")
        self.ref_encode_calls = getattr(self, "ref_encode_calls", 0) + 1
        return g

    @property
    def stft_params(self):
        """How a recording becomes this model's spectrogram (``audio.StftParams``).  Defaults to what ``spec_channels``, ``hop_length`` and
        ``sampling_rate`` imply (``StftParams.from_hparams``); assign ``StftParams.from_config(cfg)`` for a checkpoint whose ``config.json``
        says otherwise (another ``win_length``, mel limits)."""
        from . import audio
        if getattr(self, "_stft_params", None) is None:
            self._stft_params = audio.StftParams.from_hparams(self.hp)
        return self._stft_params

    @stft_params.setter
    def stft_params(self, params) -> None:
        from . import audio
        if not isinstance(params, audio.StftParams):
            raise ValueError("stft_params must be an audio.StftParams")
        if params.channels != self.hp.spec_channels:
            raise ValueError(f"these parameters give {params.channels} rows, the model reads spec_channels = {self.hp.spec_channels}")
        self._stft_params = params

    @torch.no_grad()
    def reference_embedding_from_wav(self, wav: torch.Tensor, wav_lengths=None, sampling_rate: Optional[int] = None) -> torch.Tensor:
        """The voice of a recording -> g [B, gin]: ``audio.spectrogram(wav, wav_lengths, self.stft_params)`` on the model's device, then
        ``reference_embedding`` with the frame counts it produced (a ragged batch is exact in both steps).  ``wav`` [B, S] or [S], fp32 in
        [-1, 1] or int16 PCM at ``sampling_rate`` (``None``: the model's).  A recording at another rate is resampled on the device first
        (``audio.resample``); its resampled lengths stay there, and lengths given on the host are checked as resampled."""
        from . import audio
        if self.hp.n_speakers != 0:
            raise RuntimeError("reference_embedding_from_wav needs a model built with n_speakers=0 (this one has a speaker table: emb_g)")
        wav, wav_lengths = audio.to_rate(wav, wav_lengths, sampling_rate, self.hp.sampling_rate, self.stft_params, self.device)
        spec, lengths = audio.spectrogram(wav, wav_lengths, self.stft_params, device=self.device)
        return self.reference_embedding(spec, lengths)

    # ------------------------------------------------------------------ the two phases
    @torch.no_grad()
    def encode_durations(self, x, x_lengths, sid, tone, language, bert, ja_bert, en_bert, noise_w=None, noise_scale_w=0.8,
                         sdp_ratio=0.0, length_scale=1.0, bert_index=None, g=None, lean=False, seeds=None) -> Dict[str, torch.Tensor]:
        """Phase A = reference models.py:1045-1057.  ``noise_w`` [B,2,T] is the draw of models.py:248-251.

        ``seeds`` (an int, B ints or an int64 tensor [B]; see ``infer``): the stochastic predictor's noise is computed on the device from
        each utterance's seed instead (``bv2_set_noise_seeds``); ``noise_w`` must then be None.

        ``lean`` (what ``infer`` asks for): the output the mix ``logw = sdp * r + dp * (1 - r)`` cannot see is not asked for, which lets the
        library run only the other predictor (include/bv2.h, ``bv2_encode_out``): at a scalar ``sdp_ratio`` of exactly 0 there is no
        ``logw_sdp``, the stochastic predictor is not launched and ``noise_w`` is neither uploaded nor read (it may stay on the host); at
        exactly 1 there is no ``logw_dp`` and the deterministic one is not launched.  Any other ratio or per-utterance ratios: all ten
        outputs, as in the full form.  With a tap set or ``set_option("lean_durations", 0)`` both predictors run as well.  What is returned
        is bit for bit what the full form returns (``logw``: by value, a zero may differ in sign).

        ``g`` (optional, [B, gin] or [B, gin, 1]): the speaker vectors to condition on instead of ``emb_g(sid)`` — ``sid`` is then not
        read and may be None (``bv2_encode_durations_g``).  A model with ``n_speakers=0`` has no table and needs it.

        ``bert_index`` (optional, a 3-tuple aligned with bert / ja_bert / en_bert; entries may be None): a feature with an index is
        WORD-level — [B, 1024, S] as the BERT model emitted it, still on the device — and symbol t reads column index[b, t]; the
        word2ph repeat of reference text/chinese_bert.py:48-58 happens as a gather inside the TextEncoder front
        (``bert_features.word_level_feature`` builds the pair)."""
        if self._blob is None:
            self.repack()
        dev = self.device
        B, T = x.shape
        i64 = lambda t: t.to(dev, torch.int64).contiguous()
        f32 = lambda t: t.to(dev, torch.float32).contiguous()
        if g is not None:
            g = self._speaker_vector(g, B)
            sid = None
        elif self.hp.n_speakers == 0:
            raise ValueError("this model has no speaker table (n_speakers=0): pass g (reference_embedding(y)) or, to infer(), y")
        x, x_lengths, tone, language = i64(x), i64(x_lengths), i64(tone), i64(language)
        sid = None if sid is None else i64(sid)
        if g is None and sid is None:
            raise ValueError("sid must be given (or g)")
        bert, ja_bert, en_bert = f32(bert), f32(ja_bert), f32(en_bert)
        bidx = [None, None, None] if bert_index is None else [None if t is None else t.to(dev, torch.int32).contiguous() for t in bert_index]
        for feat, ix in zip((bert, ja_bert, en_bert), bidx):
            want = (B, H.BERT_DIM, T) if ix is None else (B, H.BERT_DIM, feat.shape[2])
            if tuple(feat.shape) != want or (ix is not None and (tuple(ix.shape) != (B, T) or not 1 <= feat.shape[2] <= T)):
                raise ValueError(f"bert features must be [B,{H.BERT_DIM},T] (reference infer.py:124), or [B,{H.BERT_DIM},S<=T] with a [B,T] index")
        cols = [0 if ix is None else int(f.shape[2]) for f, ix in zip((bert, ja_bert, en_bert), bidx)]

        def with_index(ein, ptr_of):
            for i in range(3):
                ein.bert_index[i] = None if bidx[i] is None else ptr_of(i)
                ein.bert_cols[i] = cols[i]
            return ein
        seeds = item_seeds(seeds, B, dev)
        if seeds is not None and noise_w is not None:
            raise ValueError("encode_durations: seeds and noise_w exclude each other (a seeded call reads no noise tensor)")
        if seeds is None and noise_w is None:
            raise ValueError("encode_durations needs noise_w [B,2,T] (draw_noise_w) or seeds")
        if seeds is None and tuple(noise_w.shape) != (B, 2, T):
            raise ValueError("noise_w must be [B,2,T]")
        # per-utterance controls: if any of the three is a [B] tensor, all three go to the library as [B] arrays (rows 0-2 of a
        # [4, B] buffer, bv2_item_controls); otherwise the scalar call runs exactly as before
        ctrl = [item_control(n, v, B, None) for n, v in (("noise_scale_w", noise_scale_w), ("sdp_ratio", sdp_ratio),
                                                          ("length_scale", length_scale))]
        ctl = None
        if any(t is not None for _, t in ctrl):
            ctl = _control_buffer([t for _, t in ctrl])
            for r, (v, t) in enumerate(ctrl):
                if t is not None:
                    ctl[r].copy_(t)
                else:
                    ctl[r].fill_(v)
            ctl = ctl.to(dev)                                     # one upload when the values came from the host
            noise_scale_w = sdp_ratio = length_scale = 0.0        # ignored by the library: every member of the controls is set
        else:
            noise_scale_w, sdp_ratio, length_scale = (v for v, _ in ctrl)
        # the library's rule for leaving the stochastic predictor out (bv2_exec.cpp run_encode), mirrored to know whether noise_w is read
        skip_sdp = bool(lean and ctl is None and sdp_ratio == 0.0 and not self._taps and self._options.get("lean_durations", 1))
        noise_w = None if (skip_sdp or seeds is not None) else f32(noise_w)
        hp = self.hp
        e = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
        okeys = ("g", "x", "m_p", "logs_p", "x_mask", "logw_sdp", "logw_dp", "logw", "w_ceil", "y_lengths")
        # lean: the output of the predictor the mix cannot see is NULL in bv2_encode_out and absent from the result
        unseen = {0.0: "logw_sdp", 1.0: "logw_dp"}.get(sdp_ratio) if lean and ctl is None else None
        mk_out = lambda: dict(g=e(B, hp.gin_channels), x=e(B, hp.hidden_channels, T), m_p=e(B, hp.inter_channels, T),
                              logs_p=e(B, hp.inter_channels, T), x_mask=e(B, T),
                              **{k: e(B, T) for k in ("logw_sdp", "logw_dp") if k != unseen},
                              logw=e(B, T), w_ceil=e(B, T), y_lengths=torch.empty(B, dtype=torch.int64, device=dev))
        if self._graphs_on and not self._taps:
            ws = self._workspace(B, T, 1)
            ins = dict(x=x, x_lengths=x_lengths, sid=sid, tone=tone, language=language, bert=bert, ja_bert=ja_bert,
                       en_bert=en_bert, noise_w=noise_w)
            if noise_w is None:
                del ins["noise_w"]                  # not read: neither staged nor moved
            if g is not None:
                del ins["sid"]                      # not read
                ins["g"] = g                        # the graph owns a [B, gin] copy, refilled before every replay like the controls
            for i in range(3):
                if bidx[i] is not None:
                    ins[f"bert_index{i}"] = bidx[i]
            if ctl is not None:
                ins["ctl"] = ctl                    # the graph owns a [4, B] copy: its values are refilled before every replay
            if seeds is not None:
                ins["seeds"] = seeds                # the graph owns an int64 [B] copy, read at replay time: the key says "seeded", not the values

            static = self._graphs_static
            moving = ("noise_w", "ctl", "g", "seeds")

            def build(own_inputs):
                staged = tuple(ins) if own_inputs else tuple(k for k in moving if k in ins)   # static_io: the rest is read in place
                sin = {k: (torch.empty_like(v) if k in staged else v) for k, v in ins.items()}
                sout = mk_out()
                ein = L.EncodeIn(B, T, *[_ptr(sin.get(k)) for k in ("x", "x_lengths", "sid", "tone", "language", "bert", "ja_bert",
                                                                    "en_bert", "noise_w")],
                                 float(noise_scale_w), float(sdp_ratio), float(length_scale))
                with_index(ein, lambda i: sin[f"bert_index{i}"].data_ptr())
                eout = L.EncodeOut(*[_ptr(sout.get(k)) for k in okeys])
                icp = None if ctl is None else _controls_ptr(sin["ctl"], (0, 1, 2))
                with torch.cuda.device(dev), self._seeded(sin.get("seeds")):
                    if g is not None:
                        gr = self._capture(self._lib.bv2_graph_capture_encode_g, C.byref(ein), C.byref(eout), icp, _ptr(sin["g"]),
                                           C.c_void_p(ws.data_ptr()), ws.numel())
                    elif ctl is None:
                        gr = self._capture(self._lib.bv2_graph_capture_encode, C.byref(ein), C.byref(eout),
                                           C.c_void_p(ws.data_ptr()), ws.numel())
                    else:
                        gr = self._capture(self._lib.bv2_graph_capture_encode_ex, C.byref(ein), C.byref(eout), icp,
                                           C.c_void_p(ws.data_ptr()), ws.numel())
                return dict(graph=gr, sin=sin, sout=sout, staged=staged)

            ptrs = tuple(ins[k].data_ptr() for k in ins if k not in moving) if static else ()
            # per-utterance controls and a given g: the key carries the fact ("ctl" / "g" in ins), not the values
            scal = ("item",) if ctl is not None else (float(noise_scale_w), float(sdp_ratio), float(length_scale))
            ent = self._graph_entry(("A", B, T, bool(lean)) + scal + (tuple(cols), tuple(sorted(ins))), build, ptrs)
            for k in ent["staged"]:
                ent["sin"][k].copy_(ins[k], non_blocking=True)
            with torch.cuda.device(dev):
                if self._lib.bv2_graph_launch(ent["graph"], C.c_void_p(torch.cuda.current_stream().cuda_stream)):
                    raise RuntimeError("bv2_graph_launch (encode) failed")
            if static:
                return dict(ent["sout"])
            return {k: v.clone() for k, v in ent["sout"].items()}
        out = mk_out()
        ein = L.EncodeIn(B, T, _ptr(x), _ptr(x_lengths), _ptr(sid), _ptr(tone), _ptr(language), _ptr(bert), _ptr(ja_bert),
                         _ptr(en_bert), _ptr(noise_w), float(noise_scale_w), float(sdp_ratio), float(length_scale))
        with_index(ein, lambda i: bidx[i].data_ptr())
        eout = L.EncodeOut(*[_ptr(out.get(k)) for k in okeys])
        ws = self._workspace(B, T, 1)
        with torch.cuda.device(dev), self._seeded(seeds):
            stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            if g is not None:
                self._check(self._lib.bv2_encode_durations_g(self._handle, stream, C.byref(ein), C.byref(eout),
                                                             None if ctl is None else _controls_ptr(ctl, (0, 1, 2)), _ptr(g),
                                                             C.c_void_p(ws.data_ptr()), ws.numel()), "bv2_encode_durations_g")
            elif ctl is None:
                self._check(self._lib.bv2_encode_durations(self._handle, stream, C.byref(ein), C.byref(eout),
                                                           C.c_void_p(ws.data_ptr()), ws.numel()), "bv2_encode_durations")
            else:
                self._check(self._lib.bv2_encode_durations_ex(self._handle, stream, C.byref(ein), C.byref(eout),
                                                              _controls_ptr(ctl, (0, 1, 2)), C.c_void_p(ws.data_ptr()), ws.numel()),
                            "bv2_encode_durations_ex")
        return out

    @torch.no_grad()
    def decode(self, enc: Dict[str, torch.Tensor], noise_z: torch.Tensor, Ty: int, noise_scale=0.667, max_len=None,
               want_attn: bool = True, exact_lengths: bool = False, ty_bucket: Optional[int] = None, seeds=None) -> Dict[str, torch.Tensor]:
        """Phase B = reference models.py:1058-1073.  ``noise_z`` [B,inter,>=Ty] replaces randn_like at :1071.
        ``seeds`` (see ``infer``): the prior noise is computed inside the expanding kernel from each utterance's seed; ``noise_z`` must be
        None, no noise tensor exists and nothing is drawn from torch's generator.
        ``ty_bucket``: run at T_y rounded up to a multiple of it and cut the outputs back (default: the ``enable_graphs`` bucket when a
        graph is replayed, none on the eager path; tests pass it to the eager path to compare like with like)."""
        if self._blob is None:
            self.repack()
        dev = self.device
        hp = self.hp
        B, _, T = enc["x"].shape
        Ci = hp.inter_channels
        noise_scale, ns_item = item_control("noise_scale", noise_scale, B, None)
        ctl = None
        if ns_item is not None:                         # per-utterance noise_scale: row 3 of a [4, B] control buffer
            ctl = _control_buffer([ns_item])
            ctl[3].copy_(ns_item)
            ctl = ctl.to(dev)
            noise_scale = 0.0
        seeds = item_seeds(seeds, B, dev)
        if seeds is not None and noise_z is not None:
            raise ValueError("decode: seeds and noise_z exclude each other (a seeded call reads no noise tensor)")
        draw_z = noise_z is None and seeds is None      # infer(): draw #2 straight into the graph's buffer (static_io)
        if noise_z is not None:
            assert noise_z.is_cuda and noise_z.dtype == torch.float32 and noise_z.shape[2] >= Ty and noise_z.shape[1] == Ci
        L_dec = Ty if (max_len is None or max_len <= 0 or max_len >= Ty) else int(max_len)
        S = L_dec * hp.total_upsample
        okeys = ("o", "attn", "y_mask", "z", "z_p", "m_p", "logs_p")
        # ---- T_y bucket: everything below runs at Ty (the bucket); Ty_true / S_true cut the results back
        if ty_bucket is None:
            ty_bucket = self._ty_bucket if (self._graphs_on and not self._taps) else 1
        Ty_true, S_true, L_true = Ty, S, L_dec
        mode = int(bool(exact_lengths))
        if ty_bucket > 1:
            Ty = (Ty + ty_bucket - 1) // ty_bucket * ty_bucket
            if L_dec == Ty_true:                        # no max_len cut: the Generator runs over the bucket, capped on the device
                L_dec = Ty
                mode = 1 if exact_lengths else 2
            S = L_dec * hp.total_upsample
        bucketed = Ty != Ty_true

        def cut(out):
            if not bucketed:
                return out
            r = dict(out)
            r["o"] = out["o"][:, :, :S_true]
            for k in ("z", "z_p", "m_p", "logs_p", "y_mask"):
                r[k] = None if out[k] is None else out[k][:, :, :Ty_true]
            r["attn"] = None if out["attn"] is None else out["attn"][:, :, :Ty_true]
            return r

        def mk_out():
            # ONE allocation carved into the six secondary outputs (+ one for the waveform): this runs between the reference's host sync and the first launch of
            # phase B, i.e. with the GPU idle — seven caching-allocator calls there cost ~25 us of a 4.5 ms step at batch 1
            shapes = dict(o=(B, 1, S), attn=(B, 1, Ty, T) if want_attn else None, y_mask=(B, 1, Ty), z=(B, Ci, Ty), z_p=(B, Ci, Ty),
                          m_p=(B, Ci, Ty), logs_p=(B, Ci, Ty))
            # The waveform gets its OWN allocation: a caller that keeps only `o` (the serving case) must not pin attn and the four
            # [B,Ci,Ty] latents with it.
            sizes = {k: (0 if sh is None or k == "o" else (math.prod(sh) + 63) // 64 * 64) for k, sh in shapes.items()}   # 256-byte aligned views
            flat = torch.empty(sum(sizes.values()), dtype=torch.float32, device=dev)
            out, off = {"o": torch.empty(shapes["o"], dtype=torch.float32, device=dev)}, 0
            for k, sh in shapes.items():
                if k == "o":
                    continue
                out[k] = None if sh is None else flat[off:off + math.prod(sh)].view(*sh)
                off += sizes[k]
            return out
        if self._graphs_on and not self._taps:
            ws = self._workspace(B, T, Ty)
            ikeys = ("m_p", "logs_p", "x_mask", "w_ceil", "y_lengths", "g")

            static = self._graphs_static

            def build(own_inputs):
                sin = {k: (torch.empty_like(enc[k]) if own_inputs else enc[k]) for k in ikeys}
                # the reference's strides for the prior noise (draw_noise_z): an in-place normal_() on it IS randn_like(m_p)
                if seeds is None:
                    sin["noise_z"] = torch.zeros(B, Ty, Ci, dtype=torch.float32, device=dev).transpose(1, 2)   # zeros: a bucket's tail is never drawn
                else:
                    sin["seeds"] = torch.zeros_like(seeds)     # read at replay time; no noise buffer exists
                if ctl is not None:
                    sin["ctl"] = torch.zeros_like(ctl)
                sout = mk_out()
                nzs = sin.get("noise_z")
                din = L.DecodeIn(B, T, int(Ty), int(L_dec), *[_ptr(sin[k]) for k in ikeys], _ptr(nzs),
                                 *((0, 0, 0) if nzs is None else nzs.stride()), float(noise_scale), mode)
                dout = L.DecodeOut(*[_ptr(sout[k]) for k in okeys])
                with torch.cuda.device(dev), self._seeded(sin.get("seeds")):
                    if ctl is None:
                        g = self._capture(self._lib.bv2_graph_capture_decode, C.byref(din), C.byref(dout),
                                          C.c_void_p(ws.data_ptr()), ws.numel())
                    else:
                        g = self._capture(self._lib.bv2_graph_capture_decode_ex, C.byref(din), C.byref(dout),
                                          _controls_ptr(sin["ctl"], (3,)), C.c_void_p(ws.data_ptr()), ws.numel())
                return dict(graph=g, sin=sin, sout=sout)

            ptrs = tuple(enc[k].data_ptr() for k in ikeys) if static else ()
            scal = "item" if ctl is not None else float(noise_scale)   # per-utterance: the fact, not the values
            ent = self._graph_entry(("B", B, T, int(Ty), int(L_dec), bool(want_attn), scal, mode, seeds is not None), build, ptrs)
            if ent["own_inputs"]:
                for k in ikeys:
                    ent["sin"][k].copy_(enc[k])
            if ctl is not None:
                ent["sin"]["ctl"].copy_(ctl)
            if seeds is not None:
                ent["sin"]["seeds"].copy_(seeds)
            elif draw_z and not bucketed:
                ent["sin"]["noise_z"].normal_()
            elif draw_z:                                # the reference draws exactly [B, C, T_y] in its memory order (draw_noise_z): keep the RNG contract
                ent["sin"]["noise_z"][:, :, :Ty_true].copy_(draw_noise_z(B, Ci, Ty_true, dev))
            else:
                ent["sin"]["noise_z"][:, :, :Ty_true].copy_(noise_z[:, :, :Ty_true])
            with torch.cuda.device(dev):
                if self._lib.bv2_graph_launch(ent["graph"], C.c_void_p(torch.cuda.current_stream().cuda_stream)):
                    raise RuntimeError("bv2_graph_launch (decode) failed")
            if static:
                return cut(dict(ent["sout"]))
            return {k: (None if v is None else v.clone()) for k, v in cut(ent["sout"]).items()}
        if draw_z:
            noise_z = draw_noise_z(B, Ci, Ty_true, dev)
        if bucketed and seeds is None:                  # eager run at a bucket (tests): zero tail, reference-strided like the graph's buffer
            nzb = torch.zeros(B, Ty, Ci, dtype=torch.float32, device=dev).transpose(1, 2)
            nzb[:, :, :Ty_true].copy_(noise_z[:, :, :Ty_true])
            noise_z = nzb
        out = mk_out()
        din = L.DecodeIn(B, T, int(Ty), int(L_dec), _ptr(enc["m_p"]), _ptr(enc["logs_p"]), _ptr(enc["x_mask"]),
                         _ptr(enc["w_ceil"]), _ptr(enc["y_lengths"]), _ptr(enc["g"]), _ptr(noise_z),
                         *((0, 0, 0) if noise_z is None else noise_z.stride()), float(noise_scale), mode)
        dout = L.DecodeOut(*[_ptr(out[k]) for k in okeys])
        ws = self._workspace(B, T, Ty)
        with torch.cuda.device(dev), self._seeded(seeds):
            stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            if ctl is None:
                self._check(self._lib.bv2_decode(self._handle, stream, C.byref(din), C.byref(dout), C.c_void_p(ws.data_ptr()),
                                                 ws.numel()), "bv2_decode")
            else:
                self._check(self._lib.bv2_decode_ex(self._handle, stream, C.byref(din), C.byref(dout), _controls_ptr(ctl, (3,)),
                                                    C.c_void_p(ws.data_ptr()), ws.numel()), "bv2_decode_ex")
        return cut(out)

    # ------------------------------------------------------------------ the reference entry point
    @torch.no_grad()
    def infer(self, x, x_lengths, sid, tone, language, bert, ja_bert, en_bert, noise_scale=0.667, length_scale=1,
              noise_scale_w=0.8, max_len=None, sdp_ratio=0, y=None, *, g=None, y_lengths=None, noise_w=None, noise_z=None,
              w_ceil=None, want_attn=True, exact_lengths=False, bert_index=None, ty_bucket=None, w_ceil_items=None, seeds=None):
        """reference models.py:1026-1074.  Keyword-only extras (not in the reference): ``noise_w`` [B,2,T] and
        ``noise_z`` [B,inter,>=T_y] inject the two N(0,1) draws (parity tests; the reference's ONNX export externalises
        them the same way), ``w_ceil`` substitutes the durations (``w_ceil_items`` [B] bool: only for the marked items), ``want_attn=False`` skips materialising the path,
        ``exact_lengths=True`` makes every utterance of a ragged batch come out exactly as if it had been run alone (the
        reference's unmasked decoder lets the padding bleed into an utterance's last ~40 ms; bv2.h ``exact_lengths``),
        ``bert_index`` hands BERT features over at word level (see ``encode_durations``), ``ty_bucket`` runs phase B at T_y rounded up to
        a multiple of it (default: ``enable_graphs``' bucket when graphs are on, exact T_y otherwise; see ``enable_graphs``).

        ``sdp_ratio``, ``noise_scale``, ``noise_scale_w`` and ``length_scale`` each take a number (or 0-d tensor) or, as in the
        reference, one value per utterance as a tensor shaped [B], [B,1] or [B,1,1] (``item_control``): utterance b then gets what a
        batch-1 call with its own values gets (``bv2_item_controls``).  With graphs on, one capture per shape serves every set of
        per-utterance values; scalar values stay part of the graph key as before.

        The speaker (models.py:1045-1048): ``g`` ([B, gin] or [B, gin, 1]) wins if given — phase A conditions on it instead of a table
        row, through the same kernel code (``g = stage_emb_g(s)`` is bit-identical to ``sid = s``), and ``sid`` may be None.  Otherwise a
        model with ``n_speakers=0`` encodes ``y`` [B, spec_channels, L] first (``reference_embedding(y, y_lengths)``; ``y_lengths`` [B] is
        this library's addition for padded reference batches), and a model with a speaker table looks ``sid`` up and ignores ``y``, as the
        reference does.  With graphs on, ``g`` lives in a buffer the graph owns: one capture per shape serves every voice.

        ``seeds`` (an int for every item, B ints, or an int64 tensor [B]): per-utterance noise seeds.  Both draws then come from a
        counter-based generator inside the kernels that consume them (``bv2_set_noise_seeds``, csrc/kernels/rng.h): utterance b's noise
        at (draw, row, frame) depends on ``seeds[b]`` alone — not on the batch it rides in, its row, T, T_y or the bucket — torch's
        generators are not touched, and no noise tensor is made.  It excludes ``noise_w`` / ``noise_z`` (``seeded_noise`` gives the same
        values as tensors).  With graphs on the seeds live in a buffer the graph owns: one capture serves every seed."""
        if self.device.type != "cuda":
            raise RuntimeError("bert_vits2_amd.SynthesizerTrn.infer needs a GPU: no CPU fallback exists by design")
        dev = self.device
        B, T = x.shape
        seeds = item_seeds(seeds, B, dev)
        if seeds is not None and (noise_w is not None or noise_z is not None):
            raise ValueError("infer: seeds and noise_w / noise_z exclude each other")
        if g is None and self.hp.n_speakers == 0:
            if y is None:
                raise ValueError("this model has no speaker table (n_speakers=0): infer() needs y (the reference spectrogram) or g")
            g = self.reference_embedding(y, y_lengths)
        if noise_w is None and seeds is None:
            noise_w = draw_noise_w(B, T, None)         # drawn either way (the RNG stream stays the reference's); uploaded only if read
        enc = self.encode_durations(x, x_lengths, sid, tone, language, bert, ja_bert, en_bert, noise_w,
                                    noise_scale_w=noise_scale_w, sdp_ratio=sdp_ratio, length_scale=length_scale,
                                    bert_index=bert_index, g=g, lean=True, seeds=seeds)
        if w_ceil is not None:
            _substitute_durations(enc, w_ceil, w_ceil_items, B, T, dev)
        # the reference's one host sync (commons.py:120-122).  One utterance: no reduction kernel in front of the copy.
        Ty = int(enc["y_lengths"].item()) if B == 1 else int(enc["y_lengths"].max().item())
        if noise_z is not None:                        # None: decode() draws it (in place in the graph's buffer when replaying)
            noise_z = noise_z.to(dev, torch.float32)
        dec = self.decode(enc, noise_z, Ty, noise_scale=noise_scale, max_len=max_len, want_attn=want_attn,
                          exact_lengths=exact_lengths, ty_bucket=ty_bucket, seeds=seeds)
        self.last_encode = _LastEncode(enc, self, noise_w, noise_scale_w, seeds)
        return dec["o"], dec["attn"], dec["y_mask"], (dec["z"], dec["z_p"], dec["m_p"], dec["logs_p"])

    @torch.no_grad()
    def infer_stream(self, x, x_lengths, sid, tone, language, bert, ja_bert, en_bert, noise_scale=0.667, length_scale=1,
                     noise_scale_w=0.8, max_len=None, sdp_ratio=0, y=None, *, g=None, y_lengths=None, noise_w=None, noise_z=None,
                     w_ceil=None, want_attn=True, exact_lengths=False, bert_index=None, chunk_frames=64, first_chunk_frames=None,
                     as_pcm16=False, pcm_gain=32767.0, output_rate=None, w_ceil_items=None, seeds=None) -> SynthesisStream:
        """``infer`` with the audio handed out chunk by chunk (``SynthesisStream``): phase A, the host sync and the flow run here
        (``bv2_stream_begin``), the Generator runs window by window as the caller iterates — ``chunk_frames`` kept frames per chunk
        (``first_chunk_frames`` for the first one: a short first chunk is on the host sooner), each window carrying ``generator_halo``
        frames on both sides so that its kept samples are the whole decode's.  The arguments of ``infer`` mean what they mean there.
        ``as_pcm16``: chunks are int16, ``trunc(clamp(x * pcm_gain, -32768, 32767))`` — a fixed gain, not the per-utterance peak of
        ``serving.to_pcm16`` (a stream cannot know the peak).  The workspace is planned for a window, not for T_y
        (``bv2_stream_workspace_bytes``).  Graph replay and taps do not combine with a stream: it raises if either is on.
        ``output_rate``: the chunks leave at that sampling rate instead of the model's (``bv2_resample`` on a rolling device buffer, see
        ``SynthesisStream``): offsets and ``total_samples`` then count output-rate samples, a chunk that completes no output yields
        nothing, and item b is resampled as its own ``y_lengths[b] * U`` samples with ``exact_lengths``, as all ``total`` samples without."""
        if output_rate is not None and int(output_rate) != int(self.hp.sampling_rate):
            from . import audio
            audio.resample_plan(int(self.hp.sampling_rate), int(output_rate))      # ValueError naming the limit, before any work
        if self.device.type != "cuda":
            raise RuntimeError("bert_vits2_amd.SynthesizerTrn.infer_stream needs a GPU: no CPU fallback exists by design")
        if self._graphs_on:
            raise RuntimeError("infer_stream: graph replay is on (enable_graphs(False) first): a chunk's window pointer changes per call")
        if self._taps:
            raise RuntimeError("infer_stream: taps are set (set_tap(None) first)")
        chunk_frames = int(chunk_frames)
        first = chunk_frames if first_chunk_frames is None else int(first_chunk_frames)
        if chunk_frames < 1 or first < 1:
            raise ValueError("chunk_frames and first_chunk_frames must be >= 1")
        dev, hp = self.device, self.hp
        B, T = x.shape
        if g is None and hp.n_speakers == 0:
            if y is None:
                raise ValueError("this model has no speaker table (n_speakers=0): infer_stream() needs y (the reference spectrogram) or g")
            g = self.reference_embedding(y, y_lengths)
        seeds = item_seeds(seeds, B, dev)              # per-utterance noise seeds, as in infer: z_p does not depend on the chunking
        if seeds is not None and (noise_w is not None or noise_z is not None):
            raise ValueError("infer_stream: seeds and noise_w / noise_z exclude each other")
        if noise_w is None and seeds is None:
            noise_w = draw_noise_w(B, T, None)         # drawn either way (the RNG stream stays the reference's); uploaded only if read
        enc = self.encode_durations(x, x_lengths, sid, tone, language, bert, ja_bert, en_bert, noise_w,
                                    noise_scale_w=noise_scale_w, sdp_ratio=sdp_ratio, length_scale=length_scale,
                                    bert_index=bert_index, g=g, lean=True, seeds=seeds)
        if w_ceil is not None:
            _substitute_durations(enc, w_ceil, w_ceil_items, B, T, dev)
        yl_host = [int(v) for v in enc["y_lengths"].cpu()]           # the reference's one host sync; every length, for the consumer
        Ty = max(yl_host)
        Ci = hp.inter_channels
        if seeds is None:
            noise_z = draw_noise_z(B, Ci, Ty, dev) if noise_z is None else noise_z.to(dev, torch.float32)
            assert noise_z.shape[2] >= Ty and noise_z.shape[1] == Ci
        noise_scale, ns_item = item_control("noise_scale", noise_scale, B, None)
        ctl = None
        if ns_item is not None:
            ctl = _control_buffer([ns_item])
            ctl[3].copy_(ns_item)
            ctl = ctl.to(dev)
            noise_scale = 0.0
        frames = Ty if (max_len is None or max_len <= 0 or max_len >= Ty) else int(max_len)
        window = max(chunk_frames, first)
        e = lambda *sh: torch.empty(*sh, dtype=torch.float32, device=dev)
        aux = dict(attn=e(B, 1, Ty, T) if want_attn else None, y_mask=e(B, 1, Ty), z=e(B, Ci, Ty), z_p=e(B, Ci, Ty), m_p=e(B, Ci, Ty),
                   logs_p=e(B, Ci, Ty))
        nbytes = self._lib.bv2_stream_workspace_bytes(self._handle, B, T, Ty, window)
        if nbytes < 0:
            raise RuntimeError("bv2_stream_workspace_bytes failed")
        ws = torch.empty(int(nbytes), dtype=torch.uint8, device=dev)        # the stream's own: it must stay untouched until the last chunk
        din = L.DecodeIn(B, T, int(Ty), int(frames), _ptr(enc["m_p"]), _ptr(enc["logs_p"]), _ptr(enc["x_mask"]), _ptr(enc["w_ceil"]),
                         _ptr(enc["y_lengths"]), _ptr(enc["g"]), _ptr(noise_z), *((0, 0, 0) if noise_z is None else noise_z.stride()),
                         float(noise_scale), int(bool(exact_lengths)))
        dout = L.DecodeOut(None, *[_ptr(aux[k]) for k in ("attn", "y_mask", "z", "z_p", "m_p", "logs_p")])
        with torch.cuda.device(dev), self._seeded(seeds):
            self._check(self._lib.bv2_stream_begin(self._handle, C.c_void_p(torch.cuda.current_stream().cuda_stream), C.byref(din),
                                                   C.byref(dout), _controls_ptr(ctl, (3,)), C.c_void_p(ws.data_ptr()), ws.numel()),
                        "bv2_stream_begin")
        bounds, t = [], 0
        while t < frames:
            t1 = min(frames, t + (first if t == 0 else chunk_frames))
            bounds.append((t, t1))
            t = t1
        self.last_encode = _LastEncode(enc, self, noise_w, noise_scale_w, seeds)
        st = SynthesisStream(self, enc, ws, Ty, frames, bounds, window, exact_lengths, as_pcm16, pcm_gain, aux, output_rate)
        st.y_lengths_host = yl_host
        return st

    # ------------------------------------------------------------------ single stages (reference ONNX seams)
    # onnx_modules/V230/models_onnx.py:896-1063 cuts infer() into emb_g / enc_p / sdp / dp / flow / dec; the six methods below
    # are those graphs (same tensor names, see onnx_api.StageSession for the consumer-side glue).
    def _stage_call(self, fn, B, T_or_Ty, *ptr_args, what):
        ws = self._workspace(B, max(int(T_or_Ty), 1), max(int(T_or_Ty), 1))
        with torch.cuda.device(self.device):
            stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            self._check(fn(self._handle, stream, *ptr_args, C.c_void_p(ws.data_ptr()), ws.numel()), what)

    def _f32(self, t, *shape):
        t = t.to(self.device, torch.float32)
        return (t.reshape(*shape) if shape else t).contiguous()

    def _i64(self, t):
        return t.to(self.device, torch.int64).contiguous()

    @torch.no_grad()
    def stage_emb_g(self, sid: torch.Tensor) -> torch.Tensor:
        """``emb_g.run({"sid"})`` -> g [B, gin]."""
        if self._blob is None:
            self.repack()
        sid = self._i64(sid).reshape(-1)
        B = sid.shape[0]
        g = torch.empty(B, self.hp.gin_channels, dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            self._check(self._lib.bv2_stage_emb_g(self._handle, stream, B, _ptr(sid), _ptr(g)), "bv2_stage_emb_g")
        return g

    @torch.no_grad()
    def stage_enc_p(self, x, t, language, bert_0, bert_1, bert_2, g, x_lengths=None):
        """``enc.run({"x","t","language","bert_0","bert_1","bert_2","g"})`` -> (xout, m_p, logs_p, x_mask [B,1,T])."""
        if self._blob is None:
            self.repack()
        x, t, language = self._i64(x), self._i64(t), self._i64(language)
        B, T = x.shape
        b0, b1, b2 = (self._f32(v, B, H.BERT_DIM, T) for v in (bert_0, bert_1, bert_2))
        g = self._f32(g, B, -1)
        xl = None if x_lengths is None else self._i64(x_lengths)
        hp, dev = self.hp, self.device
        e = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
        xout, m_p, logs_p, x_mask = e(B, hp.hidden_channels, T), e(B, hp.inter_channels, T), e(B, hp.inter_channels, T), e(B, 1, T)
        self._stage_call(self._lib.bv2_stage_enc_p, B, T, B, T, _ptr(x), _ptr(t), _ptr(language), _ptr(b0), _ptr(b1), _ptr(b2),
                         _ptr(g), _ptr(xl), _ptr(xout), _ptr(m_p), _ptr(logs_p), _ptr(x_mask), what="bv2_stage_enc_p")
        return xout, m_p, logs_p, x_mask

    @torch.no_grad()
    def stage_sdp(self, x, x_mask, zin, g) -> torch.Tensor:
        """``sdp.run({"x","x_mask","zin","g"})`` -> logw [B,1,T]; ``zin`` [B,2,T] is the already scaled noise."""
        if self._blob is None:
            self.repack()
        B, _, T = x.shape
        x, x_mask, zin, g = self._f32(x), self._f32(x_mask, B, T), self._f32(zin, B, 2, T), self._f32(g, B, -1)
        logw = torch.empty(B, 1, T, dtype=torch.float32, device=self.device)
        self._stage_call(self._lib.bv2_stage_sdp, B, T, B, T, _ptr(x), _ptr(x_mask), _ptr(zin), _ptr(g), _ptr(logw),
                         what="bv2_stage_sdp")
        return logw

    @torch.no_grad()
    def stage_dp(self, x, x_mask, g) -> torch.Tensor:
        """``dp.run({"x","x_mask","g"})`` -> logw [B,1,T]."""
        if self._blob is None:
            self.repack()
        B, _, T = x.shape
        x, x_mask, g = self._f32(x), self._f32(x_mask, B, T), self._f32(g, B, -1)
        logw = torch.empty(B, 1, T, dtype=torch.float32, device=self.device)
        self._stage_call(self._lib.bv2_stage_dp, B, T, B, T, _ptr(x), _ptr(x_mask), _ptr(g), _ptr(logw), what="bv2_stage_dp")
        return logw

    @torch.no_grad()
    def stage_flow(self, z_p: torch.Tensor, y_lengths: Optional[torch.Tensor], g: torch.Tensor,
                   y_mask: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``flow.run({"z_p","y_mask","g"})`` -> z.  The frame mask is given as ``y_lengths`` [B] or as ``y_mask`` [B,1,Ty]."""
        if self._blob is None:
            self.repack()
        B, Ci, Ty = z_p.shape
        z_p = self._f32(z_p)
        z = torch.empty_like(z_p)
        yl = None if y_lengths is None else self._i64(y_lengths)
        ym = None if y_mask is None else self._f32(y_mask, B, Ty)
        if (yl is None) == (ym is None):
            raise ValueError("stage_flow needs exactly one of y_lengths / y_mask")
        g = self._f32(g, B, -1)
        self._stage_call(self._lib.bv2_stage_flow, B, Ty, B, Ty, _ptr(z_p), _ptr(yl), _ptr(ym), _ptr(g), _ptr(z),
                         what="bv2_stage_flow")
        return z

    @torch.no_grad()
    def stage_flow_forward(self, z: torch.Tensor, y_lengths: Optional[torch.Tensor], g: torch.Tensor,
                           y_mask: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``flow(z, y_mask, g=g)`` in the direction of the reference's ``forward()`` (models.py:958) -> z_p: a posterior latent mapped
        into the prior's space, where ``align_latent`` compares it with the text.  ``stage_flow`` undoes it.  Always fp32."""
        if self._blob is None:
            self.repack()
        B, Ci, Ty = z.shape
        z = self._f32(z)
        z_p = torch.empty_like(z)
        yl = None if y_lengths is None else self._i64(y_lengths)
        ym = None if y_mask is None else self._f32(y_mask, B, Ty)
        if (yl is None) == (ym is None):
            raise ValueError("stage_flow_forward needs exactly one of y_lengths / y_mask")
        g = self._f32(g, B, -1)
        self._stage_call(self._lib.bv2_stage_flow_forward, B, Ty, B, Ty, _ptr(z), _ptr(yl), _ptr(ym), _ptr(g), _ptr(z_p),
                         what="bv2_stage_flow_forward")
        return z_p

    @torch.no_grad()
    def stage_generator(self, z: torch.Tensor, y_lengths: Optional[torch.Tensor], g: torch.Tensor,
                        L_frames: Optional[int] = None):
        """``dec.run({"z_in","g"})`` -> o [B,1,L*hop].  With ``y_lengths`` the input is (z*y_mask)[:, :, :L] (models.py:1073);
        with ``None`` z is taken as it is (the exported graph)."""
        if self._blob is None:
            self.repack()
        B, Ci, Ty = z.shape
        Lf = Ty if L_frames is None else int(L_frames)
        z = self._f32(z)
        yl = None if y_lengths is None else self._i64(y_lengths)
        g = self._f32(g, B, -1)
        o = torch.empty(B, 1, Lf * self.hp.total_upsample, dtype=torch.float32, device=self.device)
        self._stage_call(self._lib.bv2_stage_generator, B, Ty, B, Ty, Lf, _ptr(z), _ptr(yl), _ptr(g), _ptr(o),
                         what="bv2_stage_generator")
        return o

    # ------------------------------------------------------------------ posterior encoder (reference models.py:448-487)
    POSTERIOR_HINT = _POSTERIOR.hint

    @property
    def has_posterior(self) -> bool:
        return getattr(self, "_post_blob", None) is not None

    def pack_posterior_host_blob(self, state_dict) -> torch.Tensor:
        """The ``enc_q.*`` tensors of ``state_dict`` packed into the posterior encoder's own blob (host, uint8).  CPU-only."""
        if not any(k.startswith("enc_q.") for k in state_dict):
            raise ValueError(self.POSTERIOR_HINT)
        return self._pack_kind(_POSTERIOR, state_dict.items())

    def load_posterior(self, path_or_state_dict) -> None:
        """Load the posterior encoder ``enc_q`` from a training checkpoint (a path to a ``G_*.pth``, its dict, or a plain state dict): the
        ``enc_q.*`` keys are packed into a blob of their own and attached; the inference blob is untouched.  Raises ``ValueError`` with a
        hint at ``compress_model.py`` when the checkpoint has none."""
        self._load_kind(_POSTERIOR, self.pack_posterior_host_blob(_plain_state_dict(path_or_state_dict)))

    def _need_posterior(self, what: str) -> None:
        self._need_kind(_POSTERIOR, what)

    @torch.no_grad()
    def posterior_encode(self, y, y_lengths, sid=None, g=None, noise_q=None, noise_scale_q=1.0, seeds=None) -> Dict[str, torch.Tensor]:
        """``enc_q(y, y_lengths, g=g)`` (reference models.py:957): ``y`` [B, spec_channels, Ty] the recording's linear spectrogram
        (``audio.spectrogram(wav, ..., net_g.stft_params)``), ``y_lengths`` [B]; the speaker is ``g`` [B, gin] or ``emb_g(sid)``.
        ``noise_q`` [B, inter, Ty] is the N(0, 1) draw of models.py:486, made by the caller like ``noise_w`` / ``noise_z``; ``None`` gives the
        deterministic ``z = m_q * mask``; ``seeds`` (see ``infer``) computes the draw in the sampling kernel from each item's seed instead
        (``seeded_noise(seeds, NOISE_Q, inter, Ty)`` as a tensor) and excludes ``noise_q``.  Returns ``z``, ``m_q``, ``logs_q`` [B, inter, Ty], ``y_mask`` [B, 1, Ty] and ``g``."""
        self._need_posterior("posterior_encode")
        if self._blob is None:
            self.repack()
        dev, hp = self.device, self.hp
        y = self._f32(y)
        B, S, Ty = y.shape
        if S != hp.spec_channels:
            raise ValueError(f"y must be [B, {hp.spec_channels}, Ty], got {tuple(y.shape)}")
        if g is None:
            if sid is None:
                raise ValueError("posterior_encode needs sid or g")
            g = self.stage_emb_g(sid)
        g = self._speaker_vector(g, B)
        yl = self._i64(y_lengths).reshape(B)
        nq = None
        seeds = item_seeds(seeds, B, dev)
        if seeds is not None and noise_q is not None:
            raise ValueError("posterior_encode: seeds and noise_q exclude each other")
        if noise_q is not None:
            nq = self._f32(noise_q)
            if tuple(nq.shape) != (B, hp.inter_channels, Ty):
                raise ValueError(f"noise_q must be [B, {hp.inter_channels}, Ty]")
        e = lambda *s: torch.empty(*s, dtype=torch.float32, device=dev)
        out = dict(z=e(B, hp.inter_channels, Ty), m_q=e(B, hp.inter_channels, Ty), logs_q=e(B, hp.inter_channels, Ty), y_mask=e(B, 1, Ty))
        n = self._lib.bv2_posterior_workspace_bytes(self._handle, B, Ty)
        ws = torch.empty(int(n), dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev), self._seeded(seeds):
            stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            self._check(self._lib.bv2_posterior_encode(self._handle, stream, B, Ty, _ptr(y), _ptr(yl), _ptr(g), _ptr(nq), float(noise_scale_q),
                                                       _ptr(out["z"]), _ptr(out["m_q"]), _ptr(out["logs_q"]), _ptr(out["y_mask"]),
                                                       C.c_void_p(ws.data_ptr()), ws.numel()), "bv2_posterior_encode")
        out["g"] = g
        return out

    @torch.no_grad()
    def align(self, x, x_lengths, sid, tone, language, bert, ja_bert, en_bert, y, y_lengths, g=None, noise_q=None,
              want_attn: bool = False, one_call: bool = False, seeds=None) -> Dict:
        """Text + recording -> frames per symbol, the reference's own aligner (models.py:950-991): phase A for the text's prior,
        ``posterior_encode`` and the forward flow for the recording's latent, ``neg_cent`` and ``maximum_path``.  ``y`` [B, spec_channels,
        Ty] may come straight from ``audio.spectrogram(wav, ..., net_g.stft_params)``.  ``y_lengths`` on the host (list, numpy, CPU
        tensor) are checked against ``x_lengths``.  Returns ``durations`` [B, T] int64, ``y_lengths``, ``score``, the encode dict ``enc``
        (``with_durations(out["enc"], out["durations"])`` is ready for ``decode``), the posterior dict ``posterior`` and, with
        ``want_attn``, ``attn`` and ``neg_cent``.  ``one_call``: everything behind phase A as ONE library call (``bv2_align``: same launches, one
        workspace, the intermediates stay inside it — ``posterior``, ``z_p`` and ``neg_cent`` are then not returned).  ``seeds`` (see ``infer``): the
        posterior draw comes from each item's seed (excludes ``noise_q``); the same seeds give the same durations."""
        self._need_posterior("align")
        B, T = x.shape
        seeds = item_seeds(seeds, B, self.device)
        if seeds is not None and noise_q is not None:
            raise ValueError("align: seeds and noise_q exclude each other")
        xl_host = None if (isinstance(x_lengths, torch.Tensor) and x_lengths.is_cuda) else [int(v) for v in x_lengths]
        _align.check_lengths(xl_host, y_lengths, T, int(y.shape[2]))
        if g is None and self.hp.n_speakers == 0:
            g = self.reference_embedding(y, torch.as_tensor(y_lengths))
        enc = self.encode_durations(x, torch.as_tensor(x_lengths), sid, tone, language, bert, ja_bert, en_bert, draw_noise_w(B, T, None),
                                    sdp_ratio=0.0, g=g, lean=True)          # the prior does not depend on the duration predictors
        if one_call:
            dev = self.device
            yd, yl, xl = self._f32(y), self._i64(torch.as_tensor(y_lengths)).reshape(B), self._i64(torch.as_tensor(x_lengths)).reshape(B)
            Ty = int(yd.shape[2])
            nq = None if noise_q is None else self._f32(noise_q)
            out = dict(durations=torch.empty(B, T, dtype=torch.int64, device=dev), score=torch.empty(B, dtype=torch.float32, device=dev),
                       attn=torch.empty(B, 1, Ty, T, dtype=torch.float32, device=dev) if want_attn else None, y_lengths=yl, enc=enc)
            n = self._lib.bv2_align_workspace_bytes(self._handle, B, T, Ty)
            ws = torch.empty(int(n), dtype=torch.uint8, device=dev)
            with torch.cuda.device(dev), self._seeded(seeds):
                self._check(self._lib.bv2_align(self._handle, C.c_void_p(torch.cuda.current_stream().cuda_stream), B, T, Ty, _ptr(enc["m_p"]),
                                                _ptr(enc["logs_p"]), _ptr(xl), _ptr(yd), _ptr(yl), _ptr(enc["g"]), _ptr(nq),
                                                _ptr(out["durations"]), _ptr(out["attn"]), _ptr(out["score"]), C.c_void_p(ws.data_ptr()),
                                                ws.numel()), "bv2_align")
            return out
        post = self.posterior_encode(y, torch.as_tensor(y_lengths), g=enc["g"], noise_q=noise_q, seeds=seeds)
        z_p = self.stage_flow_forward(post["z"], torch.as_tensor(y_lengths), enc["g"])
        out = _align.align_latent(enc, z_p, y_lengths, want_attn=want_attn, x_lengths=x_lengths)
        out["enc"], out["posterior"], out["z_p"] = enc, post, z_p
        return out

    # ------------------------------------------------------------------ forced alignment (reference models.py:960-991)
    @torch.no_grad()
    def align_latent(self, enc: Dict[str, torch.Tensor], z_p: torch.Tensor, y_lengths, want_attn: bool = False, x_lengths=None) -> Dict:
        """The reference's aligner on a recording's latent: ``enc`` is a phase-A encode dict of the text (``encode_durations``), ``z_p``
        [B, inter, Ty] the recording's latent in the prior's space (``flow(enc_q(y))`` of a training checkpoint), ``y_lengths`` its frames
        per item.  Returns ``durations`` [B, T] int64 (frames per symbol), ``y_lengths``, ``score`` and, with ``want_attn``, ``attn``
        [B, 1, Ty, T] and ``neg_cent`` [B, Ty, T] (``align.neg_cent`` + ``align.maximum_path``: two launches, kernels/align.hip).
        ``with_durations(enc, durations)`` is then ready for ``decode``: the text spoken with the recording's timing."""
        if tuple(z_p.shape[:2]) != (enc["m_p"].shape[0], self.hp.inter_channels):
            raise ValueError(f"z_p must be [B, {self.hp.inter_channels}, Ty] with the encode dict's B")
        return _align.align_latent(enc, z_p.to(self.device), y_lengths, want_attn=want_attn, x_lengths=x_lengths)

    # ------------------------------------------------------------------ scoring a take (reference models.py:993-1002, losses.py:45-61)
    SDP_FORWARD_HINT = _SDP_FORWARD.hint

    @property
    def has_sdp_forward(self) -> bool:
        return getattr(self, "_sdpf_blob", None) is not None

    def pack_sdp_forward_host_blob(self, state_dict) -> torch.Tensor:
        """``sdp.post_*`` and ``sdp.flows.1.*`` packed into the forward duration predictor's own blob (host, uint8).  ``sdp.flows.1.*`` is
        part of the inference schema (inference just never applies it): where ``state_dict`` does not carry it, the model's own
        parameters are packed.  CPU-only."""
        if not any(k.startswith("sdp.post_") for k in state_dict):
            raise ValueError(self.SDP_FORWARD_HINT)
        tensors = {k: v for k, v in self.state_dict().items() if k.startswith("sdp.flows.1.")}
        tensors.update(state_dict)
        return self._pack_kind(_SDP_FORWARD, tensors.items())

    def load_sdp_forward(self, path_or_state_dict) -> None:
        """Load what the stochastic duration predictor needs to run FORWARD on observed durations (``duration_nll``, ``score``) from a
        training checkpoint (a path to a ``G_*.pth``, its dict, or a plain state dict): ``sdp.post_pre / post_convs / post_proj /
        post_flows.*`` and ``sdp.flows.1.*`` go into a blob of their own; the inference and posterior blobs are untouched.  Raises
        ``ValueError`` with a hint at ``compress_model.py`` when the checkpoint has no ``sdp.post_*``."""
        self._load_kind(_SDP_FORWARD, self.pack_sdp_forward_host_blob(_plain_state_dict(path_or_state_dict)))

    def _need_sdp_forward(self, what: str) -> None:
        self._need_kind(_SDP_FORWARD, what)

    @torch.no_grad()
    def duration_nll(self, enc: Dict[str, torch.Tensor], durations, noise_e=None, seeds=None) -> Dict[str, torch.Tensor]:
        """``sdp(x, x_mask, w, g=g)`` of the reference's ``forward()`` (models.py:993, 197-244): the negative log-likelihood of
        ``durations`` [B, T] (frames per symbol: what ``align`` returns, or a caller's) under the stochastic duration predictor, given the
        text of ``enc`` (an ``encode_durations`` dict: ``x``, ``x_mask``, ``g``).  Returns ``nll`` [B] and its exact per-symbol
        decomposition ``nll_sym`` [B, T] (0 at masked positions; ``nll[b]`` is the fixed-order sum of row b).  ``noise_e`` [B, 2, T] is the
        N(0, 1) draw of models.py:214-217; ``seeds`` (see ``infer``) takes it from each item's seed instead (draw ``NOISE_E``) and excludes
        ``noise_e``; with neither it is drawn with ``torch.randn`` like ``draw_noise_w``.  Always fp32."""
        self._need_sdp_forward("duration_nll")
        if self._blob is None:
            self.repack()
        dev = self.device
        x = self._f32(enc["x"])
        B, Hc, T = x.shape
        mask, g = self._f32(enc["x_mask"], B, T), self._f32(enc["g"], B, -1)
        if Hc != self.hp.hidden_channels or g.shape[1] != self.hp.gin_channels:
            raise ValueError(f"enc must hold x [B, {self.hp.hidden_channels}, T] and g [B, {self.hp.gin_channels}] (an encode_durations dict)")
        w = torch.as_tensor(durations)
        if w.numel() != B * T:
            raise ValueError(f"durations must be [B, T] = [{B}, {T}], got {tuple(w.shape)}")
        w = self._f32(w, B, T)
        seeds = item_seeds(seeds, B, dev)
        if seeds is not None and noise_e is not None:
            raise ValueError("duration_nll: seeds and noise_e exclude each other")
        ne = None
        if seeds is None:
            ne = self._f32(draw_noise_w(B, T, None) if noise_e is None else noise_e)
            if tuple(ne.shape) != (B, 2, T):
                raise ValueError("noise_e must be [B, 2, T]")
        out = dict(nll=torch.empty(B, dtype=torch.float32, device=dev), nll_sym=torch.empty(B, T, dtype=torch.float32, device=dev))
        n = self._lib.bv2_duration_nll_workspace_bytes(self._handle, B, T)
        ws = torch.empty(int(n), dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev), self._seeded(seeds):
            stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            self._check(self._lib.bv2_duration_nll(self._handle, stream, B, T, _ptr(x), _ptr(mask), _ptr(w), _ptr(g), _ptr(ne),
                                                   _ptr(out["nll_sym"]), _ptr(out["nll"]), C.c_void_p(ws.data_ptr()), ws.numel()),
                        "bv2_duration_nll")
        return out

    @torch.no_grad()
    def score(self, x, x_lengths, sid, tone, language, bert, ja_bert, en_bert, y, y_lengths, g=None, durations=None, seeds=None,
              noise_q=None, noise_e=None) -> Dict:
        """How well the model explains a recording of a text: the two quantities the reference's ``forward()`` computes for it
        (models.py:993-1002, losses.py:45-61), decomposed.  Phase A for the text, ``posterior_encode`` and the forward flow for the
        recording ``y`` [B, spec_channels, Ty], the aligner (or the given ``durations`` [B, T]), then ``duration_nll`` and
        ``align.kl_path``.  Returns ``nll`` [B] / ``nll_sym`` [B, T] (duration likelihood per item / per symbol), ``kl`` [B] / ``kl_frame``
        [B, Ty] (the reference's ``kl_loss`` is ``kl.sum() / y_lengths.sum()``), ``durations``, ``y_lengths``, the aligner's ``score`` (None
        with given durations), and the two MSE terms of models.py:996-1002 per item, ``l_length_dp`` and ``l_length_sdp_mse``: the sum over
        the item's symbols of ``(logw - log(w + 1e-6))^2`` for the deterministic predictor and for the stochastic one run in reverse at
        noise scale 1, divided by the ITEM's symbol count (the reference divides by the batch's; at B = 1 they coincide).  Also ``enc``,
        ``posterior`` and ``z_p``.  ``seeds`` (see ``infer``) fixes all three draws (the reverse predictor's, the posterior's, ``e_q``) per
        item, so a take's score does not depend on its batch; it excludes ``noise_q`` / ``noise_e``.  Needs ``load_posterior`` and
        ``load_sdp_forward``."""
        self._need_posterior("score")
        self._need_sdp_forward("score")
        B, T = x.shape
        dev = self.device
        seeds = item_seeds(seeds, B, dev)
        if seeds is not None and (noise_q is not None or noise_e is not None):
            raise ValueError("score: seeds exclude noise_q and noise_e")
        xl_host = None if (isinstance(x_lengths, torch.Tensor) and x_lengths.is_cuda) else [int(v) for v in x_lengths]
        _align.check_lengths(xl_host, y_lengths, T, int(y.shape[2]))
        if g is None and self.hp.n_speakers == 0:
            g = self.reference_embedding(y, torch.as_tensor(y_lengths))
        # both predictors run (sdp_ratio strictly between 0 and 1, the full output set); the reverse predictor at noise scale 1 (models.py:998)
        enc = self.encode_durations(x, torch.as_tensor(x_lengths), sid, tone, language, bert, ja_bert, en_bert,
                                    None if seeds is not None else draw_noise_w(B, T, None), noise_scale_w=1.0, sdp_ratio=0.5, g=g, seeds=seeds)
        yl = torch.as_tensor(y_lengths)
        post = self.posterior_encode(y, yl, g=enc["g"], noise_q=noise_q, seeds=seeds)
        z_p = self.stage_flow_forward(post["z"], yl, enc["g"])
        xl_d = self._i64(torch.as_tensor(x_lengths)).reshape(B)
        yl_d = self._i64(yl).reshape(B)
        if durations is None:
            al = _align.align_latent(enc, z_p, y_lengths, x_lengths=x_lengths)
            dur, path_score = al["durations"], al["score"]
        else:
            dur, path_score = torch.as_tensor(durations).to(dev).reshape(B, T), None
        out = self.duration_nll(enc, dur, noise_e=noise_e, seeds=seeds)
        out.update(_align.kl_path(z_p, post["logs_q"], enc["m_p"], enc["logs_p"], dur, xl_d, yl_d))
        mask = enc["x_mask"].reshape(B, T)
        logw_ = torch.log(dur.to(torch.float32) + 1e-6) * mask
        n_sym = mask.sum(1)
        out["l_length_dp"] = ((enc["logw_dp"].reshape(B, T) - logw_) ** 2).sum(1) / n_sym
        out["l_length_sdp_mse"] = ((enc["logw_sdp"].reshape(B, T) - logw_) ** 2).sum(1) / n_sym
        out.update(durations=dur, y_lengths=yl_d, score=path_score, enc=enc, posterior=post, z_p=z_p)
        return out

    def set_option(self, key: str, value: int) -> None:
        """Kernel-selection switches of ``bv2_set_option`` ("fused_resblock", "fused_dds", "lean_durations"); tests and A/B runs."""
        self._ensure_handle()
        self._check(self._lib.bv2_set_option(self._handle, key.encode(), int(value)), "bv2_set_option")
        self._options[key] = int(value)
        self._drop_graphs()

    # ------------------------------------------------------------------ measurement
    def profile(self, on=1):
        """0 off, 1 time every MFMA kernel launch with HIP events, 2 only the Generator's launches."""
        self._ensure_handle()
        self._check(self._lib.bv2_profile_enable(self._handle, int(on)), "bv2_profile_enable")
        self._lib.bv2_profile_reset(self._handle)

    def profile_pause(self):
        """Stop recording events but keep what was recorded (the pool holds 8192 launches)."""
        self._check(self._lib.bv2_profile_enable(self._handle, 0), "bv2_profile_enable")

    def profile_report(self):
        rows = (L.ProfileRow * 256)()
        n = self._lib.bv2_profile_report(self._handle, rows, 256)
        out = []
        for i in range(max(n, 0)):
            r = rows[i]
            out.append(dict(name=r.name.decode(), launches=r.launches, total_ms=r.total_ms, flops=r.flops, bytes=r.bytes))
        self._lib.bv2_profile_reset(self._handle)
        return out


def from_hparams(hp: H.HParams) -> SynthesizerTrn:
    return SynthesizerTrn(
        hp.n_vocab, hp.spec_channels, hp.segment_size, inter_channels=hp.inter_channels, hidden_channels=hp.hidden_channels,
        filter_channels=hp.filter_channels, n_heads=hp.n_heads, n_layers=hp.n_layers, kernel_size=hp.kernel_size,
        p_dropout=hp.p_dropout, resblock=hp.resblock, resblock_kernel_sizes=hp.resblock_kernel_sizes,
        resblock_dilation_sizes=hp.resblock_dilation_sizes, upsample_rates=hp.upsample_rates,
        upsample_initial_channel=hp.upsample_initial_channel, upsample_kernel_sizes=hp.upsample_kernel_sizes,
        n_speakers=hp.n_speakers, gin_channels=hp.gin_channels, use_sdp=hp.use_sdp, n_flow_layer=hp.n_flow_layer,
        n_layers_trans_flow=hp.n_layers_trans_flow, flow_share_parameter=hp.flow_share_parameter,
        use_transformer_flow=hp.use_transformer_flow)
