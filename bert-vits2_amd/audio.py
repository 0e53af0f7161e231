"""From a recording to the spectrogram the ReferenceEncoder reads — on the device (``bv2_spectrogram``, kernels/stft.hip).

The reference turns a wav file into ``y`` with ``mel_processing.spectrogram_torch`` (reflect padding by ``(n_fft - hop) // 2``, periodic
Hann window, ``torch.stft(center=False)``, ``sqrt(re^2 + im^2 + 1e-6)``; mel_processing.py:43-78, called from data_utils.py:99-138 after
``audio / max_wav_value``), or with ``mel_spectrogram_torch`` (:95-142) for a model whose ``spec_channels`` is a mel width.  ``spectrogram``
below is that step: samples at the model's sampling rate go in (fp32 in [-1, 1], or 16-bit PCM read as ``x / 32768``), ``[B, C, L]`` comes
out.  A recording at another rate goes through ``resample`` first (the reference resamples offline with librosa, resample.py): a polyphase
Kaiser-windowed sinc on the device (``bv2_resample``, kernels/resample.hip), the same call that brings synthesised audio to the rate a
consumer wants.  ``loudness`` / ``normalize_loudness`` measure integrated loudness (ITU-R BS.1770-4, mono) and bring audio to a target level
on the device (``bv2_loudness_*``, kernels/loudness.hip); ``true_peak`` (``bv2_true_peak``, kernels/truepeak.hip), ``loudness(true_peak=,
want_range=)`` and ``normalize_loudness(peak="true")`` add the rest of an EBU R128 delivery sheet: true peak, loudness range, the maximum
momentary and short-term loudness, and a ceiling in dBTP.  ``assemble`` joins pieces that lie in several tensors, each under its level
rule, and the pauses between them into one buffer per document (``bv2_assemble``, kernels/assemble.hip).  Not done here: decoding of audio files.

Nothing in here computes: the filterbank comes from ``bv2_mel_basis`` and the resampler's table from ``bv2_resample_taps`` (fp64 on the
host, rounded to fp32), everything else runs in the two launches of ``bv2_spectrogram`` / the one of ``bv2_resample`` / the four of
``bv2_loudness_measure`` and the one of ``bv2_loudness_apply`` on the current stream.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

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


# ---- resampling (include/bv2.h bv2_resample) ---------------------------------------------------------------------------------------------
def resample_config(rate_in: int, rate_out: int, input_format: int = L.WAV_F32) -> L.ResampleConfig:
    c = L.ResampleConfig()
    c.struct_bytes = C.sizeof(L.ResampleConfig)
    c.rate_in, c.rate_out, c.input_format = int(rate_in), int(rate_out), int(input_format)
    return c


def resample_plan(rate_in: int, rate_out: int) -> Tuple[int, int, int]:
    """``(L, M, K)`` of a rate pair (``bv2_resample_plan``): ``rate_out / gcd``, ``rate_in / gcd`` and the zero crossings' reach in input
    samples (``2K + 1`` taps per phase).  ``ValueError`` outside the envelope (equal rates, a rate <= 0, ``L > 1024``, a table of more than
    2^20 entries), with the library's message."""
    lib = L.load()
    v = [C.c_int32() for _ in range(3)]
    if lib.bv2_resample_plan(C.byref(resample_config(rate_in, rate_out)), *[C.byref(x) for x in v]) != 0:
        raise ValueError(lib.bv2_last_error(None).decode())
    return tuple(int(x.value) for x in v)


def resample_length(rate_in: int, rate_out: int, n_in: int) -> int:
    """``ceil(n_in L / M)``: the samples ``n_in`` samples become."""
    Lr, M, _ = resample_plan(rate_in, rate_out)
    return -((-int(n_in) * Lr) // M)


def resample_taps(rate_in: int, rate_out: int, dtype=np.float32) -> np.ndarray:
    """The filter table ``[L, 2K + 1]`` from ``bv2_resample_taps`` — fp32 (what the device reads) or fp64 (what it was rounded from)."""
    Lr, _, K = resample_plan(rate_in, rate_out)
    lib = L.load()
    f64 = np.dtype(dtype) == np.float64
    out = np.empty((Lr, 2 * K + 1), np.float64 if f64 else np.float32)
    rc = (lib.bv2_resample_taps_f64 if f64 else lib.bv2_resample_taps)(C.byref(resample_config(rate_in, rate_out)), C.c_void_p(out.ctypes.data))
    if rc != 0:
        raise RuntimeError(f"bv2_resample_taps failed ({rc}): {lib.bv2_last_error(None).decode()}")
    return out


_TAPS: Dict[tuple, torch.Tensor] = {}


def device_taps(rate_in: int, rate_out: int, dev) -> torch.Tensor:
    """The fp32 table on ``dev``, built once per ``(rate_in, rate_out, device)`` (about 1 ms of host time)."""
    key = (int(rate_in), int(rate_out), str(torch.device(dev)))
    if key not in _TAPS:
        _TAPS[key] = torch.from_numpy(resample_taps(rate_in, rate_out)).to(dev)
    return _TAPS[key]


def resample_range(src: torch.Tensor, src_start: int, src_lengths: Optional[torch.Tensor], rate_in: int, rate_out: int, n0: int, n1: int,
                   dst: Optional[torch.Tensor] = None, dst_lengths: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The range form of ``bv2_resample`` on the current stream: ``src`` [B, n] (device, fp32 or int16, unit sample stride) holds samples
    ``[src_start, src_start + n)`` of every item, ``src_lengths`` [B] (device int64, absolute; ``None``: ``src_start + n``); outputs
    ``[n0, n1)`` go to ``dst`` [B, >= n1 - n0] (a new tensor if ``None``), ``dst_lengths`` [B] receives ``ceil(len_b L / M)``.  The caller
    keeps the two edge rules of include/bv2.h."""
    if not src.is_cuda or src.dim() != 2 or src.stride(1) != 1 or src.dtype not in (torch.float32, torch.int16):
        raise ValueError("src must be a device tensor [B, n], float32 or int16, with unit sample stride")
    B, n = src.shape
    cfg = resample_config(rate_in, rate_out, L.WAV_I16 if src.dtype == torch.int16 else L.WAV_F32)
    taps = device_taps(rate_in, rate_out, src.device)
    if dst is None:
        dst = torch.empty(B, max(int(n1) - int(n0), 0), dtype=torch.float32, device=src.device)
    lib = L.load()
    with torch.cuda.device(src.device):
        rc = lib.bv2_resample(C.c_void_p(torch.cuda.current_stream().cuda_stream), C.byref(cfg), C.c_void_p(taps.data_ptr()),
                              C.c_void_p(src.data_ptr()), src.stride(0) if B > 1 else n, int(src_start), n,
                              C.c_void_p(src_lengths.data_ptr()) if src_lengths is not None else None, B, int(n0), int(n1),
                              C.c_void_p(dst.data_ptr()), dst.stride(0) if B > 1 else dst.shape[1],
                              C.c_void_p(dst_lengths.data_ptr()) if dst_lengths is not None else None)
    if rc != 0:
        raise RuntimeError(f"bv2_resample failed ({rc}): {lib.bv2_last_error(None).decode()}")
    return dst


@torch.no_grad()
def resample(wav: torch.Tensor, wav_lengths=None, rate_in: Optional[int] = None, rate_out: Optional[int] = None, device=None
             ) -> Tuple[torch.Tensor, torch.Tensor]:
    """``wav`` [B, S] or [S] at ``rate_in`` (fp32, or int16 PCM read as ``x / 32768``; host or device, any batch stride) -> ``(out [B,
    N_max] fp32, out_lengths [B] int64)`` at ``rate_out``, both on the device; ``N_max = ceil(S L / M)``.  ``wav_lengths`` [B] (samples,
    host or device; ``None``: all S) makes a padded batch exact: item b is its own samples and zero elsewhere — the batch's padding is never
    read — it gets ``out_lengths[b] = ceil(wav_lengths[b] L / M)`` samples and zeros behind them.  Lengths given on the host are checked
    there; lengths on the device are not read back.  Equal rates: the input comes back as fp32 on the device, without a launch."""
    if rate_in is None or rate_out is None:
        raise ValueError("resample needs rate_in and rate_out")
    rate_in, rate_out = int(rate_in), int(rate_out)
    if not isinstance(wav, torch.Tensor):
        wav = torch.as_tensor(wav)
    if wav.dim() == 1:
        wav = wav[None]
    if wav.dim() != 2 or wav.shape[1] < 1 or wav.shape[0] < 1:
        raise ValueError(f"wav must be [B, S] or [S], got {tuple(wav.shape)}")
    if wav.dtype not in (torch.int16, torch.float32):
        raise ValueError(f"wav must be float32 in [-1, 1] or int16 PCM, got {wav.dtype}")
    B, S = wav.shape
    if rate_in != rate_out:
        resample_plan(rate_in, rate_out)                            # ValueError naming the limit, before anything moves
    elif rate_in < 1:
        raise ValueError(f"rates must be positive, got {rate_in}")
    if wav_lengths is not None and (not isinstance(wav_lengths, torch.Tensor) or not wav_lengths.is_cuda):
        host = [int(v) for v in torch.as_tensor(wav_lengths).reshape(-1).tolist()]
        if len(host) != B:
            raise ValueError("wav_lengths must be [B]")
        for b, n in enumerate(host):
            if not 1 <= n <= S:
                raise ValueError(f"wav_lengths[{b}] = {n} is outside [1, {S}], the samples of the batch")
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
    if rate_in == rate_out:
        out = wav.to(torch.float32) / 32768.0 if wav.dtype == torch.int16 else wav
        return out, (wl if wl is not None else torch.full((B,), S, dtype=torch.int64, device=dev))
    N = resample_length(rate_in, rate_out, S)
    lengths = torch.empty(B, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        out = resample_range(wav, 0, wl, rate_in, rate_out, 0, N, None, lengths)
    return out, lengths


# ---- loudness (include/bv2.h bv2_loudness_*) ----------------------------------------------------------------------------------------------
LOUDNESS_RATES = (8000, 192000)
PEAKS = ("sample", "true")            # what a peak ceiling limits: dBFS of the samples, or dBTP


def loudness_config(rate: int, input_format: int = L.WAV_F32) -> L.LoudnessConfig:
    c = L.LoudnessConfig()
    c.struct_bytes = C.sizeof(L.LoudnessConfig)
    c.sample_rate, c.input_format = int(rate), int(input_format)
    return c


def loudness_plan(rate: int) -> Tuple[int, int, int]:
    """``(step, block, tile)`` at a sampling rate (``bv2_loudness_plan``): ``round(rate / 10)`` samples, four steps, and the samples one
    workgroup owns.  ``ValueError`` outside 8 000 .. 192 000 Hz, with the library's message."""
    lib = L.load()
    v = [C.c_int32() for _ in range(3)]
    if lib.bv2_loudness_plan(C.byref(loudness_config(rate)), *[C.byref(x) for x in v]) != 0:
        raise ValueError(lib.bv2_last_error(None).decode())
    return tuple(int(x.value) for x in v)


def loudness_coeffs(rate: int) -> np.ndarray:
    """The K-weighting's two biquads at ``rate``: ``b0 b1 b2 a1 a2`` of the high shelf, then of the high pass (fp64, ``a0 = 1``)."""
    lib = L.load()
    out = np.empty(10, np.float64)
    if lib.bv2_loudness_coeffs(C.byref(loudness_config(rate)), C.c_void_p(out.ctypes.data)) != 0:
        raise ValueError(lib.bv2_last_error(None).decode())
    return out


def loudness_blocks(rate: int, n: int) -> int:
    """Blocks of an item of ``n`` samples (``bv2_loudness_blocks``): 0 for none, 1 below a block, else ``(n - block) // step + 1``."""
    lib = L.load()
    r = lib.bv2_loudness_blocks(C.byref(loudness_config(rate)), int(n))
    if r < 0:
        raise ValueError(lib.bv2_last_error(None).decode())
    return int(r)


def _host_groups(groups, B: int) -> Tuple[Optional[list], int]:
    """Group ids given on the host, checked there: ``[B]`` integers in ``[0, G)`` with ``G = max + 1``."""
    if groups is None:
        return None, B
    ids = [int(v) for v in torch.as_tensor(groups).reshape(-1).tolist()]
    if len(ids) != B:
        raise ValueError("groups must be [B]")
    G = max(ids) + 1
    if min(ids) < 0 or G > B:
        raise ValueError(f"group ids must lie in [0, n_groups) with n_groups <= B = {B}, got {min(ids)} .. {max(ids)}")
    return ids, G


def _loudness_input(wav, wav_lengths, rate, device):
    """The input conventions and host-side checks of ``resample``, before anything touches the device."""
    if rate is None:
        raise ValueError("loudness needs the sampling rate")
    rate = int(rate)
    if not isinstance(wav, torch.Tensor):
        wav = torch.as_tensor(wav)
    if wav.dim() == 1:
        wav = wav[None]
    if wav.dim() != 2 or wav.shape[1] < 1 or wav.shape[0] < 1:
        raise ValueError(f"wav must be [B, S] or [S], got {tuple(wav.shape)}")
    if wav.dtype not in (torch.int16, torch.float32):
        raise ValueError(f"wav must be float32 in [-1, 1] or int16 PCM, got {wav.dtype}")
    B, S = wav.shape
    loudness_plan(rate)                                            # ValueError naming the envelope
    if B > 4096:
        raise ValueError(f"loudness takes at most 4096 items per call, got {B}")
    if wav_lengths is not None and (not isinstance(wav_lengths, torch.Tensor) or not wav_lengths.is_cuda):
        host = [int(v) for v in torch.as_tensor(wav_lengths).reshape(-1).tolist()]
        if len(host) != B:
            raise ValueError("wav_lengths must be [B]")
        for b, n in enumerate(host):
            if not 1 <= n <= S:
                raise ValueError(f"wav_lengths[{b}] = {n} is outside [1, {S}], the samples of the batch")
    elif wav_lengths is not None and tuple(wav_lengths.reshape(-1).shape) != (B,):
        raise ValueError("wav_lengths must be [B]")

    def move():
        dev = torch.device(device if device is not None else
                           (wav.device if wav.is_cuda else torch.device("cuda", torch.cuda.current_device())))
        w = wav.detach().to(dev)
        if w.stride(1) != 1:
            w = w.contiguous()
        wl = None if wav_lengths is None else torch.as_tensor(wav_lengths).to(dev, torch.int64).reshape(-1).contiguous()
        return dev, w, wl
    return rate, B, S, L.WAV_I16 if wav.dtype == torch.int16 else L.WAV_F32, move


def _ptr(t: Optional[torch.Tensor]):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def loudness_measure(wav: torch.Tensor, wl: Optional[torch.Tensor], rate: int, groups: Optional[torch.Tensor] = None,
                     n_groups: Optional[int] = None, target_lufs: float = -23.0, peak_ceiling_db: float = -1.0, want_blocks: bool = False,
                     gate: bool = True) -> Dict[str, torch.Tensor]:
    """``bv2_loudness_measure`` on the current stream: ``wav`` [B, S] (device, fp32 or int16, unit sample stride), ``wl`` [B] device int64
    or ``None``, ``groups`` [B] device int32 in ``[0, n_groups)`` or ``None``.  Returns device tensors ``lufs`` fp64 [G], ``gain`` fp32
    [G], ``flags`` int32 [G], ``peak`` fp32 [B] and, if asked, ``block_ms`` fp64 [B, blocks(S)].  ``gate=False``: ``peak`` and
    ``block_ms`` only, for ``loudness_gate`` over several calls."""
    if not wav.is_cuda or wav.dim() != 2 or wav.stride(1) != 1 or wav.dtype not in (torch.float32, torch.int16):
        raise ValueError("wav must be a device tensor [B, S], float32 or int16, with unit sample stride")
    B, S = wav.shape
    dev = wav.device
    G = B if groups is None else int(n_groups)
    cfg = loudness_config(rate, L.WAV_I16 if wav.dtype == torch.int16 else L.WAV_F32)
    lib = L.load()
    n = lib.bv2_loudness_workspace_bytes(C.byref(cfg), B, S)
    if n < 0:
        raise ValueError(lib.bv2_last_error(None).decode())
    ws = torch.empty(n, dtype=torch.uint8, device=dev)
    out = {"peak": torch.empty(B, dtype=torch.float32, device=dev)}
    if gate:
        out.update(lufs=torch.empty(G, dtype=torch.float64, device=dev), gain=torch.empty(G, dtype=torch.float32, device=dev),
                   flags=torch.empty(G, dtype=torch.int32, device=dev))
    if want_blocks or not gate:
        out["block_ms"] = torch.empty(B, loudness_blocks(rate, S), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        rc = lib.bv2_loudness_measure(C.c_void_p(torch.cuda.current_stream().cuda_stream), C.byref(cfg), _ptr(wav),
                                      wav.stride(0) if B > 1 else S, _ptr(wl), B, S, _ptr(groups) if gate else None, G if gate else B,
                                      float(target_lufs), float(peak_ceiling_db), _ptr(out.get("lufs")), _ptr(out.get("gain")),
                                      _ptr(out["peak"]), _ptr(out.get("flags")), _ptr(out.get("block_ms")), _ptr(ws), ws.numel())
    if rc != 0:
        raise RuntimeError(f"bv2_loudness_measure failed ({rc}): {lib.bv2_last_error(None).decode()}")
    return out


def loudness_gate(block_ms: torch.Tensor, wl: torch.Tensor, S: int, peak: torch.Tensor, rate: int, groups: Optional[torch.Tensor],
                  n_groups: int, target_lufs: float = -23.0, peak_ceiling_db: float = -1.0) -> Dict[str, torch.Tensor]:
    """``bv2_loudness_gate`` on the current stream: gates and gains from block mean squares [B, >= blocks(S)] and peaks [B] that
    ``loudness_measure(gate=False)`` produced, possibly in several calls (rows padded to one width); ``wl`` [B] device int64."""
    B = block_ms.shape[0]
    dev = block_ms.device
    block_ms = block_ms.contiguous()
    cfg = loudness_config(rate)
    lib = L.load()
    ws = torch.empty(32 * B + 8, dtype=torch.uint8, device=dev)
    out = dict(lufs=torch.empty(n_groups, dtype=torch.float64, device=dev), gain=torch.empty(n_groups, dtype=torch.float32, device=dev),
               flags=torch.empty(n_groups, dtype=torch.int32, device=dev), peak=peak)
    with torch.cuda.device(dev):
        rc = lib.bv2_loudness_gate(C.c_void_p(torch.cuda.current_stream().cuda_stream), C.byref(cfg), _ptr(block_ms), block_ms.shape[1],
                                   _ptr(wl), B, int(S), _ptr(peak), _ptr(groups), int(n_groups), float(target_lufs),
                                   float(peak_ceiling_db), _ptr(out["lufs"]), _ptr(out["gain"]), _ptr(out["flags"]), _ptr(ws), ws.numel())
    if rc != 0:
        raise RuntimeError(f"bv2_loudness_gate failed ({rc}): {lib.bv2_last_error(None).decode()}")
    return out


def loudness_apply(wav: torch.Tensor, wl: Optional[torch.Tensor], rate: int, gain: torch.Tensor, groups: Optional[torch.Tensor] = None,
                   as_pcm16: bool = False) -> torch.Tensor:
    """``bv2_loudness_apply`` on the current stream: ``wav * gain[group]`` as fp32, or as 16-bit PCM with the fixed-gain rounding rule;
    zeros behind each item's length."""
    B, S = wav.shape
    cfg = loudness_config(rate, L.WAV_I16 if wav.dtype == torch.int16 else L.WAV_F32)
    out = torch.empty(B, S, dtype=torch.int16 if as_pcm16 else torch.float32, device=wav.device)
    lib = L.load()
    with torch.cuda.device(wav.device):
        rc = lib.bv2_loudness_apply(C.c_void_p(torch.cuda.current_stream().cuda_stream), C.byref(cfg), _ptr(wav),
                                    wav.stride(0) if B > 1 else S, _ptr(wl), B, S, _ptr(groups), gain.numel(), _ptr(gain),
                                    None if as_pcm16 else _ptr(out), _ptr(out) if as_pcm16 else None, S)
    if rc != 0:
        raise RuntimeError(f"bv2_loudness_apply failed ({rc}): {lib.bv2_last_error(None).decode()}")
    return out


def true_peak_plan(rate: int) -> Tuple[int, int]:
    """``(F, K)`` at a sampling rate (``bv2_true_peak_plan``): the oversampling factor — 4 below 96 kHz, 2 below 192 kHz, 1 at 192 kHz — and
    the interpolator's reach in input samples (36; 0 when F = 1).  ``ValueError`` outside 8 000 .. 192 000 Hz."""
    lib = L.load()
    v = [C.c_int32() for _ in range(2)]
    if lib.bv2_true_peak_plan(C.byref(loudness_config(rate)), *[C.byref(x) for x in v]) != 0:
        raise ValueError(lib.bv2_last_error(None).decode())
    return tuple(int(x.value) for x in v)


def true_peak_measure(wav: torch.Tensor, wl: Optional[torch.Tensor], rate: int) -> torch.Tensor:
    """``bv2_true_peak`` on the current stream: ``wav`` [B, S] (device, fp32 or int16, unit sample stride), ``wl`` [B] device int64 or
    ``None`` -> fp32 [B] on the device: the larger of the sample peak and the peak of the F-times oversampled signal, which is never
    written (two launches)."""
    if not wav.is_cuda or wav.dim() != 2 or wav.stride(1) != 1 or wav.dtype not in (torch.float32, torch.int16):
        raise ValueError("wav must be a device tensor [B, S], float32 or int16, with unit sample stride")
    B, S = wav.shape
    dev = wav.device
    F, _ = true_peak_plan(rate)
    cfg = loudness_config(rate, L.WAV_I16 if wav.dtype == torch.int16 else L.WAV_F32)
    lib = L.load()
    n = lib.bv2_true_peak_workspace_bytes(C.byref(cfg), B, S)
    if n < 0:
        raise ValueError(lib.bv2_last_error(None).decode())
    taps = device_taps(rate, F * rate, dev) if F > 1 else None
    ws = torch.empty(n, dtype=torch.uint8, device=dev)
    out = torch.empty(B, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        rc = lib.bv2_true_peak(C.c_void_p(torch.cuda.current_stream().cuda_stream), C.byref(cfg), _ptr(taps), _ptr(wav),
                               wav.stride(0) if B > 1 else S, _ptr(wl), B, S, _ptr(out), _ptr(ws), ws.numel())
    if rc != 0:
        raise RuntimeError(f"bv2_true_peak failed ({rc}): {lib.bv2_last_error(None).decode()}")
    return out


def limiter_config(rate: int, lookahead_ms: float = 3.0, release_ms: float = 60.0, input_format: int = L.WAV_F32) -> L.LimiterConfig:
    c = L.LimiterConfig()
    c.struct_bytes = C.sizeof(L.LimiterConfig)
    c.sample_rate, c.input_format, c.reserved = int(rate), int(input_format), 0
    c.lookahead_ms, c.release_ms = float(lookahead_ms), float(release_ms)
    return c


def limiter_plan(rate: int, lookahead_ms: float = 3.0, release_ms: float = 60.0) -> Tuple[int, int, int, int]:
    """``(H, P, F, K)`` of the limiter (``bv2_limiter_plan``): ``H = max(1, round(lookahead_ms rate / 2000))``, ``P = max(H,
    round(release_ms rate / 2000))`` and the true-peak plan's oversampling factor and reach.  ``ValueError`` outside the envelope
    (the rate, negative or non-finite times, ``H + P > lib.LIMITER_MAX_REACH``), with the library's message."""
    lib = L.load()
    v = [C.c_int32() for _ in range(4)]
    if lib.bv2_limiter_plan(C.byref(limiter_config(rate, lookahead_ms, release_ms)), *[C.byref(x) for x in v]) != 0:
        raise ValueError(lib.bv2_last_error(None).decode())
    return tuple(int(x.value) for x in v)


def limiter_window(rate: int, lookahead_ms: float = 3.0, release_ms: float = 60.0) -> np.ndarray:
    """The smoothing window ``[P + H + 1]`` fp32 from ``bv2_limiter_window``: ``w[k]`` at index ``k + P``, a half-Hann on either side of
    ``k = 0``, normalised to sum 1 in fp64 and rounded once."""
    H, P, _, _ = limiter_plan(rate, lookahead_ms, release_ms)
    lib = L.load()
    out = np.empty(P + H + 1, np.float32)
    if lib.bv2_limiter_window(C.byref(limiter_config(rate, lookahead_ms, release_ms)), C.c_void_p(out.ctypes.data)) != 0:
        raise ValueError(lib.bv2_last_error(None).decode())
    return out


_WINDOWS: Dict[tuple, torch.Tensor] = {}


def device_window(rate: int, lookahead_ms: float, release_ms: float, dev) -> torch.Tensor:
    key = (int(rate), float(lookahead_ms), float(release_ms), str(torch.device(dev)))
    if key not in _WINDOWS:
        _WINDOWS[key] = torch.from_numpy(limiter_window(rate, lookahead_ms, release_ms)).to(dev)
    return _WINDOWS[key]


def limit_apply(wav: torch.Tensor, wl: Optional[torch.Tensor], rate: int, gain: torch.Tensor, groups: Optional[torch.Tensor] = None,
                ceiling_db: float = -1.0, lookahead_ms: float = 3.0, release_ms: float = 60.0, as_pcm16: bool = False,
                want_curve: bool = False) -> Dict[str, torch.Tensor]:
    """``bv2_limit`` on the current stream (two launches): ``wav`` [B, S] (device, fp32 or int16, unit sample stride) times ``gain[group]``
    times the limiter's gain curve under a true-peak ceiling.  Returns device tensors ``out`` [B, S] (fp32, or int16 by the fixed-gain
    rule), ``min_gain`` fp32 [B], ``limited_samples`` int64 [B] and, if asked, ``curve`` fp32 [B, S]."""
    if not wav.is_cuda or wav.dim() != 2 or wav.stride(1) != 1 or wav.dtype not in (torch.float32, torch.int16):
        raise ValueError("wav must be a device tensor [B, S], float32 or int16, with unit sample stride")
    B, S = wav.shape
    dev = wav.device
    cfg = limiter_config(rate, lookahead_ms, release_ms, L.WAV_I16 if wav.dtype == torch.int16 else L.WAV_F32)
    _, _, F, _ = limiter_plan(rate, lookahead_ms, release_ms)
    lib = L.load()
    n = lib.bv2_limiter_workspace_bytes(C.byref(cfg), B, S)
    if n < 0:
        raise ValueError(lib.bv2_last_error(None).decode())
    taps = device_taps(rate, F * rate, dev) if F > 1 else None
    window = device_window(rate, lookahead_ms, release_ms, dev)
    ws = torch.empty(n, dtype=torch.uint8, device=dev)
    r = {"out": torch.empty(B, S, dtype=torch.int16 if as_pcm16 else torch.float32, device=dev),
         "min_gain": torch.empty(B, dtype=torch.float32, device=dev), "limited_samples": torch.empty(B, dtype=torch.int64, device=dev)}
    if want_curve:
        r["curve"] = torch.empty(B, S, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        rc = lib.bv2_limit(C.c_void_p(torch.cuda.current_stream().cuda_stream), C.byref(cfg), _ptr(taps), _ptr(window), _ptr(wav),
                           wav.stride(0) if B > 1 else S, _ptr(wl), B, S, _ptr(groups), gain.numel(), _ptr(gain), float(ceiling_db),
                           None if as_pcm16 else _ptr(r["out"]), _ptr(r["out"]) if as_pcm16 else None, S, _ptr(r.get("curve")),
                           _ptr(r["min_gain"]), _ptr(r["limited_samples"]), _ptr(ws), ws.numel())
    if rc != 0:
        raise RuntimeError(f"bv2_limit failed ({rc}): {lib.bv2_last_error(None).decode()}")
    return r


def loudness_steps_count(rate: int, n: int) -> int:
    """Whole 100 ms steps of an item of ``n`` samples (``bv2_loudness_steps_count``)."""
    lib = L.load()
    r = lib.bv2_loudness_steps_count(C.byref(loudness_config(rate)), int(n))
    if r < 0:
        raise ValueError(lib.bv2_last_error(None).decode())
    return int(r)


def loudness_steps(wav: torch.Tensor, wl: Optional[torch.Tensor], rate: int, want_blocks: bool = False) -> Dict[str, torch.Tensor]:
    """``bv2_loudness_steps`` on the current stream: ``step_ss`` fp64 [B, steps(S)], the K-weighted energy of every whole 100 ms step
    (zeros behind an item's last one) and, with ``want_blocks``, ``peak`` and ``block_ms`` as ``loudness_measure(gate=False)`` gives
    them (four step energies added in order and divided by the block ARE ``block_ms``, bit for bit)."""
    if not wav.is_cuda or wav.dim() != 2 or wav.stride(1) != 1 or wav.dtype not in (torch.float32, torch.int16):
        raise ValueError("wav must be a device tensor [B, S], float32 or int16, with unit sample stride")
    B, S = wav.shape
    dev = wav.device
    cfg = loudness_config(rate, L.WAV_I16 if wav.dtype == torch.int16 else L.WAV_F32)
    lib = L.load()
    n = lib.bv2_loudness_workspace_bytes(C.byref(cfg), B, S)
    if n < 0:
        raise ValueError(lib.bv2_last_error(None).decode())
    ws = torch.empty(n, dtype=torch.uint8, device=dev)
    width = loudness_steps_count(rate, S)
    out = {"step_ss": torch.empty(B, max(width, 1), dtype=torch.float64, device=dev)[:, :width]}     # S below a step: [B, 0]
    if want_blocks:
        out["peak"] = torch.empty(B, dtype=torch.float32, device=dev)
        out["block_ms"] = torch.empty(B, loudness_blocks(rate, S), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        rc = lib.bv2_loudness_steps(C.c_void_p(torch.cuda.current_stream().cuda_stream), C.byref(cfg), _ptr(wav),
                                    wav.stride(0) if B > 1 else S, _ptr(wl), B, S, C.c_void_p(out["step_ss"].data_ptr()), max(width, 1),
                                    _ptr(out.get("peak")), _ptr(out.get("block_ms")), _ptr(ws), ws.numel())
    if rc != 0:
        raise RuntimeError(f"bv2_loudness_steps failed ({rc}): {lib.bv2_last_error(None).decode()}")
    return out


def loudness_range(step_ss: torch.Tensor, wl: Optional[torch.Tensor], S: int, rate: int, groups: Optional[torch.Tensor] = None,
                   n_groups: Optional[int] = None) -> Dict[str, torch.Tensor]:
    """``bv2_loudness_range`` on the current stream (EBU Tech 3342): from step energies [B, >= steps(S)] that ``loudness_steps`` produced,
    possibly in several calls (rows padded to one width).  Returns device tensors [G]: ``lra`` (LU), ``st_low`` / ``st_high`` (LUFS at the
    10th and 95th percentile of the gated short-term loudness), ``max_short_term``, ``max_momentary`` (LUFS), all fp64, and ``flags``
    int32 (``lib.RANGE_SHORT``: no whole 3 s block; ``lib.RANGE_SILENT``: nothing above -70 LUFS; then ``lra`` is 0 and the rest -inf)."""
    B = step_ss.shape[0]
    dev = step_ss.device
    G = B if groups is None else int(n_groups)
    width = loudness_steps_count(rate, S)
    if step_ss.dtype != torch.float64 or step_ss.shape[1] < width:
        raise ValueError(f"step_ss must be float64 [B, >= {width}]")
    if step_ss.shape[1] == 0:
        step_ss = torch.zeros(B, 1, dtype=torch.float64, device=dev)
    step_ss = step_ss.contiguous()
    cfg = loudness_config(rate)
    lib = L.load()
    n = lib.bv2_loudness_range_workspace_bytes(C.byref(cfg), B, int(S))
    if n < 0:
        raise ValueError(lib.bv2_last_error(None).decode())
    ws = torch.empty(n, dtype=torch.uint8, device=dev)
    keys = ("lra", "st_low", "st_high", "max_short_term", "max_momentary")
    out = {k: torch.empty(G, dtype=torch.float64, device=dev) for k in keys}
    out["flags"] = torch.empty(G, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        rc = lib.bv2_loudness_range(C.c_void_p(torch.cuda.current_stream().cuda_stream), C.byref(cfg), _ptr(step_ss), step_ss.shape[1],
                                    _ptr(wl), B, int(S), _ptr(groups), G, *[_ptr(out[k]) for k in keys], _ptr(out["flags"]), _ptr(ws),
                                    ws.numel())
    if rc != 0:
        raise RuntimeError(f"bv2_loudness_range failed ({rc}): {lib.bv2_last_error(None).decode()}")
    return out


def _device_groups(groups, ids, dev) -> Optional[torch.Tensor]:
    if groups is None:
        return None
    if ids is not None:
        return torch.tensor(ids, dtype=torch.int32, device=dev)
    return groups.to(dev, torch.int32).reshape(-1).contiguous()


def _groups_arg(groups, B):
    """Host ids are checked here; ids on the device are the caller's word (``n_groups = B`` is then the safe size of the outputs)."""
    if isinstance(groups, torch.Tensor) and groups.is_cuda:
        if tuple(groups.reshape(-1).shape) != (B,):
            raise ValueError("groups must be [B]")
        return None, B
    return _host_groups(groups, B)


@torch.no_grad()
def loudness(wav, wav_lengths=None, rate: Optional[int] = None, groups=None, want_blocks: bool = False, device=None,
             true_peak: bool = False, want_range: bool = False) -> Dict[str, torch.Tensor]:
    """Integrated loudness (ITU-R BS.1770-4, mono) of ``wav`` [B, S] or [S] at ``rate`` — fp32, or int16 PCM read as ``x / 32768``; host
    or device, any batch stride; ``wav_lengths`` as in ``resample`` (the padding is never read).  Returns device tensors: ``lufs`` fp64
    [G] (``-inf`` for a group with no block above -70 LUFS), ``peak`` fp32 [B] (sample peak), ``silent`` bool [G] and, with
    ``want_blocks``, ``block_ms`` fp64 [B, blocks(S)] (the block mean squares, ``-0.691 + 10 log10`` of which is the momentary curve).
    ``groups`` [B]: items with one id are the pieces of one programme and are measured together; ``None``: every item on its own, G = B.
    An item shorter than 400 ms is one block of its own length.
    ``true_peak``: adds ``true_peak`` fp32 [B] (``audio.true_peak``).  ``want_range`` (EBU Tech 3342): adds ``lra`` (LU), ``st_low``,
    ``st_high``, ``max_short_term``, ``max_momentary`` (LUFS), fp64 [G], and ``range_short`` bool [G] (no whole 3 s block: ``lra`` 0, the
    rest ``-inf``; a group with nothing above -70 LUFS reads the same and is ``silent``).  The measurement then runs once, as
    ``loudness_steps`` followed by ``loudness_gate`` and ``loudness_range``; ``lufs`` and ``block_ms`` are the same bits either way."""
    rate, B, S, _, move = _loudness_input(wav, wav_lengths, rate, device)
    ids, G = _groups_arg(groups, B)
    dev, w, wl = move()
    g = _device_groups(groups, ids, dev)
    if want_range:
        st = loudness_steps(w, wl, rate, want_blocks=True)
        lens = wl if wl is not None else torch.full((B,), S, dtype=torch.int64, device=dev)
        m = loudness_gate(st["block_ms"], lens, S, st["peak"], rate, g, G)
        m["block_ms"] = st["block_ms"]
    else:
        m = loudness_measure(w, wl, rate, g, G, want_blocks=want_blocks)
    out = {"lufs": m["lufs"], "peak": m["peak"], "silent": (m["flags"] & L.LOUDNESS_SILENT) != 0}
    if want_blocks:
        out["block_ms"] = m["block_ms"]
    if true_peak:
        out["true_peak"] = true_peak_measure(w, wl, rate)
    if want_range:
        r = loudness_range(st["step_ss"], wl, S, rate, g, G)
        out.update({k: r[k] for k in ("lra", "st_low", "st_high", "max_short_term", "max_momentary")})
        out["range_short"] = (r["flags"] & L.RANGE_SHORT) != 0
    return out


@torch.no_grad()
def true_peak(wav, wav_lengths=None, rate: Optional[int] = None, device=None) -> torch.Tensor:
    """True peak (ITU-R BS.1770-4 annex 2) of ``wav`` [B, S] or [S] at ``rate``, fp32 [B] on the device; input handling as ``loudness``.
    It is ``max(|wav|.max(), |resample(wav, rate, F * rate)|.max())`` to the bit — F = 4 below 96 kHz, 2 below 192 kHz, 1 at 192 kHz —
    without the oversampled signal ever being written.  Amplitude, not dB: ``20 log10`` of it is dBTP."""
    rate, B, S, _, move = _loudness_input(wav, wav_lengths, rate, device)
    dev, w, wl = move()
    return true_peak_measure(w, wl, rate)


NO_CEILING_DB = 1000.0                # a ceiling no peak times gain reaches: the gate's gain to the target alone
MAKEUP_PASSES = (0, 3)


def _limiter_args(rate, B, lookahead_ms, release_ms, makeup_passes=0):
    """The limiter's host-side checks, before anything touches the device."""
    limiter_plan(rate, lookahead_ms, release_ms)                   # ValueError naming the envelope
    if B > 65535:
        raise ValueError(f"the limiter takes at most 65535 items per call, got {B}")
    if int(makeup_passes) != makeup_passes or not MAKEUP_PASSES[0] <= makeup_passes <= MAKEUP_PASSES[1]:
        raise ValueError(f"makeup_passes must be an integer in [{MAKEUP_PASSES[0]}, {MAKEUP_PASSES[1]}], got {makeup_passes!r}")


def min_gain_db(min_gain: torch.Tensor) -> torch.Tensor:
    return 20.0 * torch.log10(min_gain.to(torch.float64))


def limit_to_target(w: torch.Tensor, wl: Optional[torch.Tensor], rate: int, gain: torch.Tensor, g: Optional[torch.Tensor], G: int,
                    target_lufs: float, ceiling_db: float, lookahead_ms: float, release_ms: float, makeup_passes: int, as_pcm16: bool,
                    measure=None) -> Tuple[torch.Tensor, Dict[str, torch.Tensor]]:
    """The limiter under a loudness target, on the current stream and without a host sync: limit ``w * gain[group]``, measure the output,
    and ``makeup_passes`` times raise the gain by what the limiter took and limit the ORIGINAL input again.  ``measure(out) -> lufs [G]``
    measures an output (default: ``loudness_measure`` with these groups).  Returns ``(out, {gain, lufs_out, limited, min_gain_db,
    limited_samples})``; a group whose output is silent keeps its gain."""
    if measure is None:
        def measure(o):
            return loudness_measure(o, wl, rate, g, G)["lufs"]
    for left in range(int(makeup_passes), -1, -1):
        r = limit_apply(w, wl, rate, gain, g, ceiling_db, lookahead_ms, release_ms, as_pcm16 and left == 0)
        lufs_out = measure(r["out"])
        if left:
            up = torch.pow(10.0, (float(target_lufs) - lufs_out) / 20.0)
            gain = torch.where(torch.isfinite(up), gain.to(torch.float64) * up, gain.to(torch.float64)).to(torch.float32)
    hit = (r["limited_samples"] > 0).to(torch.int64)
    if g is not None:
        hit = torch.zeros(G, dtype=torch.int64, device=w.device).index_add_(0, g.to(torch.int64).clamp(0, G - 1), hit)
    return r["out"], {"gain": gain, "lufs_out": lufs_out, "limited": hit > 0, "min_gain_db": min_gain_db(r["min_gain"]),
                      "limited_samples": r["limited_samples"]}


@torch.no_grad()
def limit(wav, wav_lengths=None, rate: Optional[int] = None, gain=None, ceiling_db: float = -1.0, lookahead_ms: float = 3.0,
          release_ms: float = 60.0, groups=None, as_pcm16: bool = False, want_curve: bool = False, device=None
          ) -> Tuple[torch.Tensor, Dict[str, torch.Tensor]]:
    """Look-ahead true-peak limiter (include/bv2.h ``bv2_limit``): ``(out [B, S], info)`` on the device.  ``out = (wav * gain[group]) *
    s``, with the gain curve ``s`` at most 1 and below 1 only around crests whose TRUE peak, after the static gain, would pass
    ``ceiling_db`` (dBTP): it starts to move ``H + P + 1`` samples before a crest and is back at 1 as many behind it, ``H`` / ``P``
    from ``lookahead_ms`` / ``release_ms`` (``limiter_plan``).  ``|out| <= c (1 + 3 * 2^-24)`` by construction; an item that never
    reaches the ceiling leaves as ``loudness_apply`` writes it, bit for bit.  Input handling as ``loudness``; ``gain``: ``None`` (1), a
    number, or fp32 [G] indexed by ``groups`` ([B] when ``groups`` is ``None``).  ``info``: ``min_gain_db`` fp64 [B] (0 where nothing
    was limited), ``min_gain`` fp32 [B], ``limited_samples`` int64 [B] and, with ``want_curve``, ``curve`` fp32 [B, S]."""
    rate, B, S, _, move = _loudness_input(wav, wav_lengths, rate, device)
    ids, G = _groups_arg(groups, B)
    if not np.isfinite(ceiling_db):
        raise ValueError("ceiling_db must be finite")
    _limiter_args(rate, B, lookahead_ms, release_ms)
    dev, w, wl = move()
    g = _device_groups(groups, ids, dev)
    if gain is None or isinstance(gain, (int, float)):
        gain = torch.full((G,), 1.0 if gain is None else float(gain), dtype=torch.float32, device=dev)
    else:
        gain = torch.as_tensor(gain).to(dev, torch.float32).reshape(-1).contiguous()
        if gain.numel() < G:
            raise ValueError(f"gain must hold one value per group ({G}), got {gain.numel()}")
    r = limit_apply(w, wl, rate, gain, g, ceiling_db, lookahead_ms, release_ms, as_pcm16, want_curve)
    info = {"min_gain_db": min_gain_db(r["min_gain"]), "min_gain": r["min_gain"], "limited_samples": r["limited_samples"]}
    if want_curve:
        info["curve"] = r["curve"]
    return r["out"], info


@torch.no_grad()
def normalize_loudness(wav, wav_lengths=None, rate: Optional[int] = None, target_lufs: float = -23.0, peak_ceiling_db: float = -1.0,
                       groups=None, as_pcm16: bool = False, device=None, peak: str = "sample", limiter: bool = False,
                       lookahead_ms: float = 3.0, release_ms: float = 60.0, makeup_passes: int = 1
                       ) -> Tuple[torch.Tensor, Dict[str, torch.Tensor]]:
    """``wav`` brought to ``target_lufs``: ``(out [B, S], info)`` on the device.  Every group gets ONE static gain ``10^((target - L) /
    20)``, lowered to ``ceiling / peak`` where the group's sample peak would pass ``peak_ceiling_db`` (``info["limited"]``); a silent
    group keeps gain 1.  ``out = wav * gain`` is one fp32 multiply (zeros behind each item's length); ``as_pcm16``: int16
    ``trunc(clamp(v * 32767))`` of that product, the fixed-gain rule of streamed PCM.  ``info``: ``lufs`` fp64 [G], ``gain_db`` fp64 [G],
    ``gain`` fp32 [G] (the factor that was applied), ``peak`` fp32 [B], ``limited`` and ``silent`` bool [G].
    ``peak="true"``: the ceiling is in dBTP — the gain is lowered where the group's TRUE peak (``audio.true_peak``) would pass it, which
    is what EBU R128 asks for; ``info`` gains ``true_peak`` fp32 [B] and ``info["peak"]`` stays the sample peak.
    ``limiter=True``: the target holds.  The gate is asked for the gain to the target WITHOUT the ceiling and the look-ahead limiter
    (``audio.limit``) enforces ``peak_ceiling_db`` instead, always as a true-peak ceiling; ``peak=`` then only selects what ``info``
    reports.  Limiting removes energy, so the output is measured again and the gain becomes ``g * 10^((target - L_out) / 20)`` — on the
    device, no host sync — and the limiter runs again from the ORIGINAL input, ``makeup_passes`` times (0 .. 3).  ``info`` gains
    ``lufs_out`` fp64 [G] (the loudness of what is returned), ``min_gain_db`` fp64 [B] and ``limited_samples`` int64 [B];
    ``info["limited"]`` then means "the limiter engaged on the group".  A silent group keeps gain 1 and passes through."""
    if peak not in PEAKS:
        raise ValueError(f"peak must be one of {PEAKS}, got {peak!r}")
    rate, B, S, _, move = _loudness_input(wav, wav_lengths, rate, device)
    ids, G = _groups_arg(groups, B)
    if not (np.isfinite(target_lufs) and np.isfinite(peak_ceiling_db)):
        raise ValueError("target_lufs and peak_ceiling_db must be finite")
    if limiter:
        _limiter_args(rate, B, lookahead_ms, release_ms, makeup_passes)
    dev, w, wl = move()
    g = _device_groups(groups, ids, dev)
    if limiter:
        m0 = loudness_measure(w, wl, rate, gate=False)
        lens = wl if wl is not None else torch.full((B,), S, dtype=torch.int64, device=dev)
        m = loudness_gate(m0["block_ms"], lens, S, m0["peak"], rate, g, G, target_lufs, NO_CEILING_DB)
        out, lim = limit_to_target(w, wl, rate, m["gain"], g, G, target_lufs, peak_ceiling_db, lookahead_ms, release_ms, makeup_passes,
                                   as_pcm16)
        info = loudness_info(dict(m, gain=lim["gain"]))
        info.update(limited=lim["limited"], lufs_out=lim["lufs_out"], min_gain_db=lim["min_gain_db"],
                    limited_samples=lim["limited_samples"])
        if peak == "true":
            info["true_peak"] = true_peak_measure(w, wl, rate)
        return out, info
    if peak == "true":
        m0 = loudness_measure(w, wl, rate, gate=False)
        tp = true_peak_measure(w, wl, rate)
        lens = wl if wl is not None else torch.full((B,), S, dtype=torch.int64, device=dev)
        m = loudness_gate(m0["block_ms"], lens, S, tp, rate, g, G, target_lufs, peak_ceiling_db)
        out = loudness_apply(w, wl, rate, m["gain"], g, as_pcm16)
        info = loudness_info(dict(m, peak=m0["peak"]))
        info["true_peak"] = tp
        return out, info
    m = loudness_measure(w, wl, rate, g, G, target_lufs, peak_ceiling_db)
    out = loudness_apply(w, wl, rate, m["gain"], g, as_pcm16)
    return out, loudness_info(m)


def loudness_info(m: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    return {"lufs": m["lufs"], "gain_db": 20.0 * torch.log10(m["gain"].to(torch.float64)), "gain": m["gain"], "peak": m["peak"],
            "limited": (m["flags"] & L.LOUDNESS_LIMITED) != 0, "silent": (m["flags"] & L.LOUDNESS_SILENT) != 0}


# ---- documents (include/bv2.h bv2_assemble) ------------------------------------------------------------------------------------------------
LEVELS = {"none": L.LEVEL_NONE, "piece": L.LEVEL_PIECE_PEAK, "group": L.LEVEL_GROUP_PEAK, "gain": L.LEVEL_GAIN}


@dataclass(frozen=True)
class Piece:
    """Row ``row`` of ``sources[source]``: its first ``lengths[source][row] * hop`` samples (at most the row's S)."""
    source: int
    row: int
    group: int = 0
    doc: int = 0


@dataclass(frozen=True)
class Silence:
    samples: int
    doc: int = 0


def pause_samples(rate: int, seconds: float) -> int:
    """``int(rate * seconds)``: the reference's pause (webui.py:171, 191), at ``rate`` instead of its hardcoded 44100."""
    return int(int(rate) * float(seconds))


def paragraph_pause_samples(rate: int, interval_between_para: float, interval_between_sent: float) -> int:
    """What follows a paragraph's last sentence IN ADDITION to the sentence pause (webui.py:193-197): ``int(rate * (para - sent))`` where
    that difference is positive, else nothing."""
    extra = float(interval_between_para) - float(interval_between_sent)
    return int(int(rate) * extra) if extra > 0 else 0


def assemble_config(level: str, as_pcm16: bool, max_capacity: int = 0) -> L.AssembleConfig:
    if level not in LEVELS:
        raise ValueError(f"level must be one of {sorted(LEVELS)}, got {level!r}")
    c = L.AssembleConfig()
    c.struct_bytes = C.sizeof(L.AssembleConfig)
    c.output_format, c.level, c.max_capacity = (L.WAV_I16 if as_pcm16 else L.WAV_F32), LEVELS[level], int(max_capacity)
    return c


def assemble_plan(table, n_groups: int, n_docs: int, level: str = "piece", as_pcm16: bool = True) -> Tuple[List[int], int]:
    """``bv2_assemble_plan`` over a host table (a ctypes array of ``lib.AssembleSegment``): ``(capacity per document, tile)``.
    ``ValueError`` with the library's message for a table it refuses."""
    lib = L.load()
    cap = (C.c_int64 * max(int(n_docs), 1))()
    tile = C.c_int32()
    if lib.bv2_assemble_plan(C.byref(assemble_config(level, as_pcm16)), table, len(table), int(n_groups), int(n_docs), cap, C.byref(tile)) != 0:
        raise ValueError(lib.bv2_last_error(None).decode())
    return [int(v) for v in cap[:int(n_docs)]], int(tile.value)


def _segment_table(sources, lengths, segments):
    """The host table of ``assemble`` and its ``(n_groups, n_docs)``; every check that needs no device is made here."""
    if len(segments) < 1:
        raise ValueError("assemble needs at least one segment")
    if len(lengths) != len(sources):
        raise ValueError("lengths takes one entry per source: a device int64 tensor [B], (tensor, hop), or None")
    rows = []
    for k, (w, ln) in enumerate(zip(sources, lengths)):
        if not isinstance(w, torch.Tensor) or not w.is_cuda or w.dim() != 2 or w.dtype != torch.float32 or w.shape[1] < 1 or \
                (w.shape[1] > 1 and w.stride(1) != 1):
            raise ValueError(f"sources[{k}] must be a device float32 tensor [B, S] with unit sample stride")
        t, hop = ln if isinstance(ln, tuple) else (ln, 1)
        if t is not None and (not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.int64 or t.dim() != 1
                              or t.shape[0] != w.shape[0] or (t.shape[0] > 1 and t.stride(0) != 1)):
            raise ValueError(f"lengths[{k}] must be a dense device int64 tensor [{w.shape[0]}]")
        if int(hop) < 1:
            raise ValueError(f"lengths[{k}]: hop must be >= 1, got {hop}")
        rows.append((w, t, int(hop)))
    table = (L.AssembleSegment * len(segments))()
    n_groups = n_docs = 1
    for i, (sg, e) in enumerate(zip(segments, table)):
        if isinstance(sg, Piece):
            if not 0 <= sg.source < len(rows):
                raise ValueError(f"segment {i}: source {sg.source} is outside [0, {len(rows)})")
            w, t, hop = rows[sg.source]
            if not 0 <= sg.row < w.shape[0]:
                raise ValueError(f"segment {i}: row {sg.row} is outside [0, {w.shape[0]})")
            e.src = w.data_ptr() + 4 * sg.row * w.stride(0)
            e.length = None if t is None else t.data_ptr() + 8 * sg.row
            e.samples, e.hop, e.group = int(w.shape[1]), hop, int(sg.group)
        elif isinstance(sg, Silence):
            e.src, e.length, e.samples, e.hop, e.group = None, None, int(sg.samples), 1, 0
        else:
            raise ValueError(f"segment {i} must be an audio.Piece or an audio.Silence")
        e.doc = int(sg.doc)
        n_groups, n_docs = max(n_groups, e.group + 1), max(n_docs, e.doc + 1)
    return table, n_groups, n_docs


@torch.no_grad()
def assemble(sources: Sequence[torch.Tensor], lengths: Sequence, segments: Sequence, *, level: str = "piece", gain: Optional[torch.Tensor] = None,
             as_pcm16: bool = True, out: Optional[Sequence[torch.Tensor]] = None
             ) -> Tuple[List[torch.Tensor], torch.Tensor, torch.Tensor]:
    """``bv2_assemble`` on the current stream.  ``sources[k]`` [B_k, S_k] device fp32; ``lengths[k]`` a device int64 tensor [B_k] (samples),
    ``(tensor, hop)`` (the tensor counts frames of ``hop`` samples) or ``None`` (every row whole).  ``segments``: ``Piece(source, row,
    group, doc)`` / ``Silence(samples, doc)`` in timeline order, documents non-decreasing.  ``level``: ``"piece"`` (each piece under its own
    peak, the reference), ``"group"`` (under its group's peak), ``"gain"`` (``x * gain[group]``, ``gain`` fp32 [n_groups] on the device or
    ``None`` = 1) or ``"none"``; 16-bit PCM or fp32.  Returns ``(buffers, offsets, totals)`` on the device: one 1-D buffer per document of
    its CAPACITY (the lengths live on the device: only the first ``totals[d]`` samples are written), ``offsets`` int64 [n_segments] (each
    segment's start inside its document) and ``totals`` int64 [n_docs].  ``out``: the caller's buffers, one per document, at least its
    capacity long.  Bad input raises ``ValueError`` before any device call."""
    table, n_groups, n_docs = _segment_table(sources, lengths, segments)
    capacity, _ = assemble_plan(table, n_groups, n_docs, level, as_pcm16)
    if gain is not None:
        if level != "gain":
            raise ValueError("gain goes with level='gain'")
        if not isinstance(gain, torch.Tensor) or not gain.is_cuda or gain.dtype != torch.float32 or gain.dim() != 1 or gain.shape[0] < n_groups \
                or (gain.shape[0] > 1 and gain.stride(0) != 1):
            raise ValueError(f"gain must be a dense device float32 tensor of at least n_groups = {n_groups} entries")
    dev = sources[0].device if len(sources) else torch.device("cuda", torch.cuda.current_device())     # a timeline of pauses only
    dtype = torch.int16 if as_pcm16 else torch.float32
    if out is not None:
        if len(out) != n_docs:
            raise ValueError(f"out takes one buffer per document ({n_docs})")
        for d, (b, cap) in enumerate(zip(out, capacity)):
            if not isinstance(b, torch.Tensor) or not b.is_cuda or b.dtype != dtype or b.dim() != 1 or b.shape[0] < cap or \
                    (b.shape[0] > 1 and b.stride(0) != 1):
                raise ValueError(f"out[{d}] must be a dense 1-D device {dtype} tensor of at least {cap} samples")
        buffers = list(out)
    else:
        buffers = [torch.empty(cap, dtype=dtype, device=dev) for cap in capacity]
    lib = L.load()
    cfg = assemble_config(level, as_pcm16, max(capacity))
    n = len(table)
    nws = lib.bv2_assemble_workspace_bytes(C.byref(cfg), n, n_groups, n_docs)
    if nws < 0:
        raise ValueError(lib.bv2_last_error(None).decode())
    # one upload: the table, then the documents' base pointers and capacities
    tb = C.sizeof(L.AssembleSegment) * n
    host = np.empty(tb + 16 * n_docs, np.uint8)
    host[:tb] = np.frombuffer(table, np.uint8)
    host[tb:].view(np.int64)[:] = [b.data_ptr() for b in buffers] + capacity
    blob = torch.from_numpy(host).to(dev)
    ws = torch.empty(nws, dtype=torch.uint8, device=dev)
    offsets = torch.empty(n, dtype=torch.int64, device=dev)
    totals = torch.empty(n_docs, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        rc = lib.bv2_assemble(C.c_void_p(torch.cuda.current_stream().cuda_stream), C.byref(cfg), C.c_void_p(blob.data_ptr()), n, n_groups,
                              n_docs, _ptr(gain), C.c_void_p(blob.data_ptr() + tb), C.c_void_p(blob.data_ptr() + tb + 8 * n_docs),
                              _ptr(offsets), _ptr(totals), _ptr(ws), ws.numel())
    if rc != 0:
        raise RuntimeError(f"bv2_assemble failed ({rc}): {lib.bv2_last_error(None).decode()}")
    return buffers, offsets, totals


def to_rate(wav, wav_lengths, sampling_rate: Optional[int], model_rate: int, params: StftParams, device):
    """A recording at ``sampling_rate`` as ``(wav, wav_lengths)`` at ``model_rate`` for ``spectrogram``: untouched when the rates agree
    (or ``sampling_rate`` is ``None``), else ``resample``d on the device.  The resampled lengths stay on the device; where the caller's
    lengths were on the host (or absent) the checks ``spectrogram`` would make there are made here, on the resampled lengths."""
    if sampling_rate is None or int(sampling_rate) == int(model_rate):
        return wav, wav_lengths
    on_host = wav_lengths is None or not isinstance(wav_lengths, torch.Tensor) or not wav_lengths.is_cuda
    out, lengths = resample(wav, wav_lengths, int(sampling_rate), int(model_rate), device=device)
    if on_host:
        given = [torch.as_tensor(wav).shape[-1]] if wav_lengths is None else torch.as_tensor(wav_lengths).reshape(-1).tolist()
        for n in given:
            params.frames(resample_length(sampling_rate, model_rate, int(n)))      # ValueError naming the minimum, pad + 1
    return out, (lengths if wav_lengths is not None else None)
