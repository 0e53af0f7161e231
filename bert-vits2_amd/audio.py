"""From a recording to the spectrogram the ReferenceEncoder reads — on the device (``bv2_spectrogram``, kernels/stft.hip).

The reference turns a wav file into ``y`` with ``mel_processing.spectrogram_torch`` (reflect padding by ``(n_fft - hop) // 2``, periodic
Hann window, ``torch.stft(center=False)``, ``sqrt(re^2 + im^2 + 1e-6)``; mel_processing.py:43-78, called from data_utils.py:99-138 after
``audio / max_wav_value``), or with ``mel_spectrogram_torch`` (:95-142) for a model whose ``spec_channels`` is a mel width.  ``spectrogram``
below is that step: samples at the model's sampling rate go in (fp32 in [-1, 1], or 16-bit PCM read as ``x / 32768``), ``[B, C, L]`` comes
out.  Not done here: resampling (the reference resamples offline, resample.py) and decoding of audio files.

Nothing in here computes: the filterbank comes from ``bv2_mel_basis`` (fp64 on the host, rounded to fp32 as the reference rounds
librosa's), everything else runs in the two launches of ``bv2_spectrogram`` on the current stream.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from . import lib as L

N_FFT = (1024, 2048)          # what kernels/stft.hip transforms (the two linear widths of hparams.ENVELOPE["spec_channels"])


@dataclass(frozen=True)
class StftParams:
    """The ``data`` block of a reference ``config.json`` as far as the spectrogram needs it.  ``n_mels = 0``: linear, ``n_fft // 2 + 1`` rows."""
    n_fft: int = 2048
    hop: int = 512
    win: int = 2048
    n_mels: int = 0
    sampling_rate: int = 44100
    fmin: float = 0.0
    fmax: Optional[float] = None

    def __post_init__(self):
        if self.n_fft not in N_FFT:
            raise ValueError(f"n_fft must be one of {N_FFT}, got {self.n_fft}")
        if not 1 <= self.hop <= self.n_fft:
            raise ValueError(f"hop must be in [1, n_fft = {self.n_fft}], got {self.hop}")
        if not 1 <= self.win <= self.n_fft:
            raise ValueError(f"win must be in [1, n_fft = {self.n_fft}], got {self.win}")
        if self.n_mels < 0:
            raise ValueError(f"n_mels must not be negative, got {self.n_mels}")
        if self.n_mels and (self.sampling_rate < 1 or self.fmin < 0 or (self.fmax is not None and self.fmax <= self.fmin)):
            raise ValueError("a mel spectrogram needs sampling_rate >= 1 and 0 <= fmin < fmax")

    @property
    def pad(self) -> int:
        return (self.n_fft - self.hop) // 2

    @property
    def min_samples(self) -> int:
        """The shortest waveform that has a frame: ``pad + 1`` (reflect padding needs ``pad < n``), or one whole frame after padding where
        that is more (``hop > n_fft / 3``)."""
        return max(self.pad + 1, self.n_fft - 2 * self.pad)

    @property
    def channels(self) -> int:
        return self.n_mels if self.n_mels else self.n_fft // 2 + 1

    def frames(self, n_samples: int) -> int:
        """Frames of a waveform of ``n_samples`` (``bv2_stft_frames``); ``ValueError`` below ``min_samples``."""
        n = L.load().bv2_stft_frames(C.byref(self.config()), int(n_samples))
        if n < 0:
            raise ValueError(f"a waveform needs at least {self.min_samples} samples (pad + 1 = {self.pad + 1} for the reflect padding by "
                             f"pad = {self.pad}, and one whole frame of n_fft = {self.n_fft} after it), got {int(n_samples)}")
        return int(n)

    def config(self, input_format: int = L.WAV_F32) -> L.StftConfig:
        c = L.StftConfig()
        c.struct_bytes = C.sizeof(L.StftConfig)
        c.n_fft, c.hop, c.win, c.n_mels, c.input_format = self.n_fft, self.hop, self.win, self.n_mels, input_format
        return c

    @classmethod
    def from_hparams(cls, hp) -> "StftParams":
        """What a model's ``spec_channels`` implies: 1025 / 513 are linear spectrograms (``n_fft = 2 (spec_channels - 1)``, ``win = n_fft``),
        80 is the reference's ``use_mel_posterior_encoder`` (``n_fft`` 2048, 80 mels, fmin 0, fmax None)."""
        spec = int(hp.spec_channels)
        if spec == 80:
            return cls(2048, int(hp.hop_length), 2048, 80, int(hp.sampling_rate), 0.0, None)
        n_fft = 2 * (spec - 1)
        if n_fft not in N_FFT:
            raise ValueError(f"spec_channels = {spec} is neither a linear width of n_fft in {N_FFT} nor the mel width 80")
        return cls(n_fft, int(hp.hop_length), n_fft, 0, int(hp.sampling_rate))

    @classmethod
    def from_config(cls, cfg: dict, mel: bool = False) -> "StftParams":
        """From a reference ``config.json`` (the whole dict or its ``data`` block).  ``mel``: the 80-wide form (``n_mel_channels`` rows)."""
        d = cfg.get("data", cfg)
        return cls(int(d["filter_length"]), int(d["hop_length"]), int(d["win_length"]), int(d["n_mel_channels"]) if mel else 0,
                   int(d["sampling_rate"]), float(d.get("mel_fmin", 0.0) or 0.0), d.get("mel_fmax"))


def mel_basis(params: StftParams, dtype=np.float32) -> np.ndarray:
    """``librosa.filters.mel(sampling_rate, n_fft, n_mels, fmin, fmax)`` (Slaney scale, Slaney norm) ``[n_mels, n_fft // 2 + 1]`` from
    ``bv2_mel_basis`` — fp32 (what the device reads) or fp64 (what it was rounded from)."""
    if params.n_mels < 1:
        raise ValueError("mel_basis needs n_mels >= 1")
    lib = L.load()
    f64 = np.dtype(dtype) == np.float64
    out = np.empty((params.n_mels, params.n_fft // 2 + 1), np.float64 if f64 else np.float32)
    fn = lib.bv2_mel_basis_f64 if f64 else lib.bv2_mel_basis
    rc = fn(C.byref(params.config()), params.sampling_rate, float(params.fmin), float(params.fmax or 0.0), C.c_void_p(out.ctypes.data))
    if rc != 0:
        raise RuntimeError(f"bv2_mel_basis failed ({rc}): {lib.bv2_last_error(None).decode()}")
    return out


_BASIS: Dict[tuple, torch.Tensor] = {}


def _device_basis(params: StftParams, dev: torch.device) -> torch.Tensor:
    key = (params, str(dev))
    if key not in _BASIS:
        _BASIS[key] = torch.from_numpy(mel_basis(params)).to(dev)
    return _BASIS[key]


@torch.no_grad()
def spectrogram(wav: torch.Tensor, wav_lengths=None, params: Optional[StftParams] = None, device=None
                ) -> Tuple[torch.Tensor, torch.Tensor]:
    """``wav`` [B, S] or [S], fp32 in [-1, 1] or int16 PCM, on the host or the device, any batch stride -> ``(spec [B, C, L], spec_lengths
    [B])``, both on the device (``device``, default: the waveform's if it is on one, else the current one).  ``wav_lengths`` [B] (samples;
    ``None``: all S) makes a padded batch exact: item b's frames are cut from its own samples reflect-padded at its own ends, frames past
    ``spec_lengths[b]`` are zeros, and the batch's padding is never read.  Lengths given on the host are checked there; lengths on the
    device are not read back (an item of ``pad`` samples or fewer then gets length 0 and zero rows).

    ``spec`` is the ``[B, C, L]`` VIEW of ``[B, L, C]`` memory: a frame's C values are one contiguous run for the kernel's stores, and
    ``reference_embedding`` reads any strides (the ReferenceEncoder's first act is that transpose)."""
    params = params or StftParams()
    if not isinstance(wav, torch.Tensor):
        wav = torch.as_tensor(wav)
    if wav.dim() == 1:
        wav = wav[None]
    if wav.dim() != 2 or wav.shape[1] < 1 or wav.shape[0] < 1:
        raise ValueError(f"wav must be [B, S] or [S], got {tuple(wav.shape)}")
    if wav.dtype == torch.int16:
        fmt = L.WAV_I16
    elif wav.dtype == torch.float32:
        fmt = L.WAV_F32
    else:
        raise ValueError(f"wav must be float32 in [-1, 1] or int16 PCM, got {wav.dtype}")
    B, S = wav.shape
    Lf = params.frames(S)
    if wav_lengths is not None:
        if not isinstance(wav_lengths, torch.Tensor) or not wav_lengths.is_cuda:
            host = [int(v) for v in torch.as_tensor(wav_lengths).reshape(-1).tolist()]
            if len(host) != B:
                raise ValueError("wav_lengths must be [B]")
            for b, n in enumerate(host):
                if n > S:
                    raise ValueError(f"wav_lengths[{b}] = {n} exceeds the {S} samples of the batch")
                params.frames(n)                                   # ValueError naming the minimum, pad + 1
    if device is None:
        device = wav.device if wav.is_cuda else torch.device("cuda", torch.cuda.current_device())
    dev = torch.device(device)
    wav = wav.detach().to(dev)
    if wav.stride(1) != 1:
        wav = wav.contiguous()
    wl = None
    if wav_lengths is not None:
        wl = torch.as_tensor(wav_lengths).to(dev, torch.int64).reshape(-1).contiguous()
        if wl.shape != (B,):
            raise ValueError("wav_lengths must be [B]")
    lib = L.load()
    cfg = params.config(fmt)
    n = lib.bv2_stft_workspace_bytes(C.byref(cfg), B, S)
    if n < 0:
        raise RuntimeError("bv2_stft_workspace_bytes failed: " + lib.bv2_last_error(None).decode())
    ws = torch.empty(n, dtype=torch.uint8, device=dev)
    Cn = params.channels
    mem = torch.empty(B, Lf, Cn, dtype=torch.float32, device=dev)
    spec = mem.transpose(1, 2)
    lengths = torch.empty(B, dtype=torch.int64, device=dev)
    basis = _device_basis(params, dev) if params.n_mels else None
    strides = (C.c_int64 * 3)(*spec.stride())
    with torch.cuda.device(dev):
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        rc = lib.bv2_spectrogram(stream, C.byref(cfg), C.c_void_p(wav.data_ptr()), wav.stride(0) if B > 1 else S,
                                 C.c_void_p(wl.data_ptr()) if wl is not None else None, B, S,
                                 C.c_void_p(basis.data_ptr()) if basis is not None else None, C.c_void_p(mem.data_ptr()), strides,
                                 C.c_void_p(lengths.data_ptr()), C.c_void_p(ws.data_ptr()), ws.numel())
    if rc != 0:
        raise RuntimeError(f"bv2_spectrogram failed ({rc}): {lib.bv2_last_error(None).decode()}")
    return spec, lengths
