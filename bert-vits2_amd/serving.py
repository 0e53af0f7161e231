"""Batched serving glue around ``SynthesizerTrn.infer``.

The reference synthesises the pieces of a request one at a time at batch 1 — ``infer.infer`` (infer.py:268-332) per
sentence / per ``|``-separated piece (webui.py:66-135, hiyoriUI.py:319-349), ``torch.cuda.empty_cache()`` after each —
then converts to 16-bit on the host.  Nothing in ``infer()`` couples batch elements, so here the
pieces of one or many requests are padded into length-bucketed batches, run through ONE ``infer()`` per bucket, cut back
to their own lengths on the device (with ``exact_lengths`` every utterance gets exactly the audio it gets alone, although
the reference's decoder is unmasked), and (optionally) converted to 16-bit PCM on the device (``bv2_pcm16``) before the
single device->host copy.  Multi-GPU: ``sharding.shard_indices`` picks this rank's utterances first.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import math
from dataclasses import InitVar, dataclass
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import hparams as H


@dataclass
class Utterance:
    """One piece as reference ``infer.get_text`` (infer.py:107-152) produces it: 1-D ids and ``[1024, T]`` features.  The four
    synthesis controls are the request's own sliders (hiyoriUI ``/voice``: sdp_ratio, noise, noisew, length); ``None`` takes the value
    ``synthesize`` was called with.  The voice is ``sid`` (a row of the speaker table) unless the utterance carries ``g`` (a speaker vector
    ``[gin]``: a cached ``reference_embedding``, a blend of table rows) or ``ref_spec`` (a reference spectrogram ``[spec_channels, L]`` for a
    model built with ``n_speakers=0``; utterances that share one tensor object share one encoding).  ``durations`` (frames per symbol, one
    per phone: what ``align.maximum_path`` returns for a recording of the same text) replaces the predicted durations after phase A — the
    utterance is spoken with that timing and comes back with exactly ``sum(durations) * hop`` samples; ``sdp_ratio``, ``noise_scale_w``
    and ``length_scale`` then change nothing for it.  Graph replay (``enable_graphs``) supports it: the substitution happens between the
    two captured phases.  ``seed`` (an int in the int64 range) makes the utterance's noise its own: both draws come from the seeded
    generator (``SynthesizerTrn.infer(seeds=...)``), so the same utterance with the same seed gets the same noise whatever it is batched
    with, whichever bucket, lane or chunking serves it."""
    phones: torch.Tensor
    tones: torch.Tensor
    lang_ids: torch.Tensor
    bert: torch.Tensor
    ja_bert: torch.Tensor
    en_bert: torch.Tensor
    sid: int = 0
    sdp_ratio: Optional[float] = None
    noise_scale: Optional[float] = None
    noise_scale_w: Optional[float] = None
    length_scale: Optional[float] = None
    g: Optional[torch.Tensor] = None
    ref_spec: Optional[torch.Tensor] = None
    # np.ndarray or Tensor [T], whole non-negative numbers.  An init-only argument that __post_init__ validates and stores as an attribute:
    # the dataclass FIELDS still end with g, ref_spec (callers that build an Utterance positionally or walk its fields see what they saw)
    durations: InitVar[Optional[object]] = None
    seed: InitVar[Optional[int]] = None                # init-only like durations: validated, then stored as an attribute (int or None)

    def __post_init__(self, durations=None, seed=None):
        self.seed = None
        if seed is not None:
            if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not -2 ** 63 <= int(seed) < 2 ** 63:
                raise ValueError("seed must be an int in the int64 range")
            self.seed = int(seed)
        if self.g is not None and (not isinstance(self.g, torch.Tensor) or self.g.dim() != 1 or self.g.shape[0] < 1):
            raise ValueError("g must be a 1-D tensor [gin]")
        if self.ref_spec is not None and (not isinstance(self.ref_spec, torch.Tensor) or self.ref_spec.dim() != 2
                                          or min(self.ref_spec.shape) < 1):
            raise ValueError("ref_spec must be a 2-D tensor [spec_channels, L]")
        if self.g is not None and self.ref_spec is not None:
            raise ValueError("an utterance carries g or ref_spec, not both")
        T = int(self.phones.shape[0])
        if self.tones.shape != (T,) or self.lang_ids.shape != (T,):
            raise ValueError("phones / tones / lang_ids must be 1-D with the same length")
        for f in (self.bert, self.ja_bert, self.en_bert):
            if tuple(f.shape) != (H.BERT_DIM, T):                     # the reference asserts the same (infer.py:124)
                raise ValueError(f"bert features must be [{H.BERT_DIM}, {T}], got {tuple(f.shape)}")
        self.durations = None
        if durations is not None:
            d = torch.as_tensor(durations).detach().cpu()
            if d.dim() != 1 or d.shape[0] != T:
                raise ValueError(f"durations must be 1-D with one entry per phone ({T}), got {tuple(d.shape)}")
            d64 = d.to(torch.float64)
            if not bool(torch.isfinite(d64).all()) or bool((d64 < 0).any()) or bool((d64 != d64.round()).any()):
                raise ValueError("durations must be whole, non-negative frame counts")
            if float(d64.sum()) < 1:
                raise ValueError("durations must sum to at least one frame")
            self.durations = d64.to(torch.float32)          # [T] on the host, as phase B reads w_ceil

    @property
    def length(self) -> int:
        return int(self.phones.shape[0])


def plan_batches(lengths: Sequence[int], max_batch: int = 32, max_pad_ratio: float = 1.25,
                 weights: Optional[Sequence[float]] = None) -> List[List[int]]:
    """Length-bucketed batches: utterances sorted by length, a batch is closed when it is full or when its longest
    member would exceed ``max_pad_ratio`` x its shortest (padding is wasted work: every kernel runs over B x T_max).
    ``weights`` (optional, one per utterance): plan on ``length x weight`` instead — with per-utterance ``length_scale`` that is
    the expected frame count, which sizes the Generator (most of the work); None keeps the plan on symbols."""
    if max_batch < 1:
        raise ValueError("max_batch must be >= 1")
    if weights is not None:
        if len(weights) != len(lengths):
            raise ValueError("weights must have one entry per utterance")
        lengths = [float(n) * float(w) for n, w in zip(lengths, weights)]
    order = sorted(range(len(lengths)), key=lambda i: (lengths[i] if weights is not None else int(lengths[i]), i))
    batches, cur = [], []
    for i in order:
        if cur and (len(cur) >= max_batch or lengths[i] > max_pad_ratio * lengths[cur[0]]):
            batches.append(cur)
            cur = []
        cur.append(i)
    if cur:
        batches.append(cur)
    return batches


def collate(utts: Sequence[Utterance], device) -> dict:
    """Zero-pad to the longest utterance of the batch (padded symbols are masked out by ``x_lengths``)."""
    B, T = len(utts), max(u.length for u in utts)
    out = dict(x=torch.zeros(B, T, dtype=torch.int64), tone=torch.zeros(B, T, dtype=torch.int64),
               language=torch.zeros(B, T, dtype=torch.int64), x_lengths=torch.tensor([u.length for u in utts], dtype=torch.int64),
               sid=torch.tensor([u.sid for u in utts], dtype=torch.int64),
               bert=torch.zeros(B, H.BERT_DIM, T), ja_bert=torch.zeros(B, H.BERT_DIM, T), en_bert=torch.zeros(B, H.BERT_DIM, T))
    for i, u in enumerate(utts):
        n = u.length
        out["x"][i, :n], out["tone"][i, :n], out["language"][i, :n] = u.phones, u.tones, u.lang_ids
        out["bert"][i, :, :n], out["ja_bert"][i, :, :n], out["en_bert"][i, :, :n] = u.bert, u.ja_bert, u.en_bert
    return {k: v.to(device, non_blocking=True) for k, v in out.items()}


def speaker_vectors(model, utts: Sequence[Utterance]) -> List[Optional[torch.Tensor]]:
    """Per utterance its speaker vector ``[gin]`` on the model's device, or None where the utterance keeps ``sid``.  The DISTINCT
    ``ref_spec`` objects of the call are encoded once, as one ragged batch (``reference_embedding`` with ``y_lengths``: each reference
    gets exactly the g it gets alone)."""
    gin, spec, dev = model.hp.gin_channels, model.hp.spec_channels, model.device
    out: List[Optional[torch.Tensor]] = [None] * len(utts)
    refs, slot = [], {}
    for i, u in enumerate(utts):
        if u.g is not None:
            if tuple(u.g.shape) != (gin,):
                raise ValueError(f"utterance {i}: g must be [{gin}], got {tuple(u.g.shape)}")
            out[i] = u.g.detach().to(dev, torch.float32)
        elif u.ref_spec is not None:
            if u.ref_spec.shape[0] != spec:
                raise ValueError(f"utterance {i}: ref_spec must be [{spec}, L], got {tuple(u.ref_spec.shape)}")
            if id(u.ref_spec) not in slot:
                slot[id(u.ref_spec)] = len(refs)
                refs.append(u.ref_spec)
        elif model.hp.n_speakers == 0:
            raise ValueError(f"utterance {i}: this model has no speaker table (n_speakers=0), the utterance needs g or ref_spec")
    if refs:
        lens = [int(r.shape[1]) for r in refs]
        y = torch.zeros(len(refs), spec, max(lens), dtype=torch.float32, device=dev)
        for k, r in enumerate(refs):
            y[k, :, :lens[k]] = r.to(dev, torch.float32)
        gs = model.reference_embedding(y, torch.tensor(lens, dtype=torch.int64))
        for i, u in enumerate(utts):
            if u.g is None and u.ref_spec is not None:
                out[i] = gs[slot[id(u.ref_spec)]]
    return out


def reference_spectrogram(model, wav: torch.Tensor, sampling_rate: Optional[int] = None) -> torch.Tensor:
    """One recording (``[S]`` or ``[1, S]``, fp32 in [-1, 1] or int16 PCM at ``sampling_rate``; ``None``: the model's) -> its spectrogram
    ``[spec_channels, L]`` on the model's device (``audio.spectrogram`` with ``model.stft_params``, after ``audio.resample`` where the
    rates differ), to be put into ``Utterance(ref_spec=...)``: utterances that share the returned tensor object share one encoding."""
    from . import audio
    wav = torch.as_tensor(wav)
    if wav.dim() == 2 and wav.shape[0] == 1:
        wav = wav[0]
    if wav.dim() != 1:
        raise ValueError(f"reference_spectrogram takes one recording [S], got {tuple(wav.shape)}")
    wav, _ = audio.to_rate(wav, None, sampling_rate, model.hp.sampling_rate, model.stft_params, model.device)
    spec, _ = audio.spectrogram(wav, None, model.stft_params, device=model.device)
    return spec[0]


def pcm16(model, wave: torch.Tensor, y_lengths: torch.Tensor, hop: Optional[int] = None) -> torch.Tensor:
    """Device-side 16-bit conversion of ``wave`` [B,1,S] (peak-normalised per utterance over its valid samples, the
    semantics of gradio ``convert_to_16_bit_wav`` used by reference webui.py:86) -> int16 [B,S].  Item b's valid samples are the first
    ``y_lengths[b] * hop``; ``hop`` defaults to the model's samples per frame (``hop = 1``: lengths in samples, as after a resampling)."""
    lib = model._ensure_handle()
    B, _, S = wave.shape
    wave = wave.contiguous()
    out = torch.empty(B, S, dtype=torch.int16, device=wave.device)
    peak = torch.empty(B, dtype=torch.int32, device=wave.device)
    yl = y_lengths.to(wave.device, torch.int64).contiguous()
    with torch.cuda.device(wave.device):
        rc = lib.bv2_pcm16(C.c_void_p(torch.cuda.current_stream().cuda_stream), C.c_void_p(wave.data_ptr()), S,
                           C.c_void_p(yl.data_ptr()), model.hp.total_upsample if hop is None else int(hop), B, S,
                           C.c_void_p(out.data_ptr()), S,
                           C.c_void_p(peak.data_ptr()))
    if rc:
        raise RuntimeError(f"bv2_pcm16 failed ({rc})")
    return out


def replicas(model, n: int) -> list:
    """``n`` shim instances that share ``model``'s packed weight blob (one copy in HBM), each with its own C handle, workspace and
    HIP stream: the unit of request-level concurrency.  A request's phase A and flow are chains of small kernels that leave most CUs
    idle; with a second request in flight on another stream its Generator fills them (batch-1 requests: 938 -> 1 265 audio-s/s with
    two in flight, 1 510 with four on MI355X, ``bench.py``'s ``config2_*_requests_in_flight``).  Cached on the model."""
    from . import models as _models
    if model.device.type != "cuda":
        raise RuntimeError("bert_vits2_amd.serving needs the model on a GPU: there is no CPU fallback")
    if model._blob is None:
        model.repack()
    reps = getattr(model, "_serving_replicas", None)
    if reps is None or getattr(model, "_serving_replicas_device", None) != model.device:
        # the cache belongs to ONE device: after model.to(another GPU) the old streams (and the replicas' handles) are on the wrong one
        reps = [(model, torch.cuda.Stream(model.device))]
    while len(reps) < n:
        with torch.device("meta"):                       # a replica only holds a handle: no CPU parameter set is materialised for it
            m = _models.from_hparams(model.hp)
        m.attach_blob(model._blob)
        reps.append((m, torch.cuda.Stream(model.device)))
    for m, _ in reps[1:]:                                # replicas follow the weights, precision switches and options of the model they serve
        if m._blob is not model._blob:
            m.attach_blob(model._blob)
        # the setters drop captured graphs: only call them on a real change (both flow variants have an fp16 form)
        if m.generator_dtype != model.generator_dtype:
            m.set_generator_dtype(model.generator_dtype)
        if m.flow_dtype != model.flow_dtype:
            m.set_flow_dtype(model.flow_dtype)
        for key, val in getattr(model, "_options", {}).items():
            if getattr(m, "_options", {}).get(key) != val:
                m.set_option(key, val)
        if (m._graphs_on, m._graphs_static) != (model._graphs_on, model._graphs_static):
            m.enable_graphs(model._graphs_on, static_io=model._graphs_static)
    model._serving_replicas, model._serving_replicas_device = reps, model.device
    return reps[:n]


@torch.no_grad()
def synthesize(model, utts: Sequence[Utterance], *, sdp_ratio=0.5, noise_scale=0.6, noise_scale_w=0.9, length_scale=1.0,
               max_batch: int = 32, max_pad_ratio: float = 1.25, as_pcm16: bool = False,
               noise: Optional[Sequence] = None, requests_in_flight: int = 1, output_rate: Optional[int] = None,
               target_lufs: Optional[float] = None, peak_ceiling_db: float = -1.0, loudness_groups: Optional[Sequence] = None,
               return_levels: bool = False, peak: str = "sample", limiter: bool = False, lookahead_ms: float = 3.0,
               release_ms: float = 60.0, makeup_passes: int = 1) -> List[np.ndarray]:
    """Synthesise every utterance; returns one 1-D array per utterance in input order (float32 like reference
    infer.py:315-319, or int16 with ``as_pcm16``).  Defaults are the reference web UI's (webui.py:443-454).
    ``noise`` (tests): per utterance a pair ``(noise_w [2,T], noise_z [inter, >= T_y])`` to inject instead of drawing.
    An utterance with a ``seed`` draws its noise from the seeded generator: its audio then does not depend on the other requests of the
    call (up to the round-off between batch shapes, INTEGRATION.md "Seeds"); ``noise=`` together with a seeded utterance raises.
    ``requests_in_flight`` > 1: the buckets are dealt round-robin to that many ``replicas`` (own handle + HIP stream, shared
    weights), so one bucket's small-kernel phases overlap another's Generator; results do not depend on it.
    An utterance that carries its own ``sdp_ratio`` / ``noise_scale`` / ``noise_scale_w`` / ``length_scale`` gets it inside the
    shared batch (per-utterance controls, one value per batch item); the call's values fill in the rest.  Buckets are then planned
    on expected frames (symbols x length_scale).  Voices: utterances with ``g`` or ``ref_spec`` are conditioned on that vector, the
    others on their ``sid`` row, all in the same buckets (``speaker_vectors``).
    ``output_rate``: audio at that sampling rate instead of the model's — every bucket is resampled on the device (``audio.resample`` over
    each utterance's own ``y_lengths * hop`` samples) before its one device-to-host copy; an utterance of n model-rate samples comes back
    with ``ceil(n L / M)``, and ``as_pcm16`` normalises by the peak of the resampled samples.
    ``target_lufs``: every utterance leaves at that integrated loudness (ITU-R BS.1770-4, ``audio.normalize_loudness``): each bucket is
    measured and scaled on the device before its one copy — after the resampling, at the output rate — by one static gain per utterance,
    lowered where the sample peak would pass ``peak_ceiling_db``; ``as_pcm16`` is then the fixed-gain 16-bit form of the normalised audio
    (``trunc(clamp(x * 32767))``), not the peak-normalised one.  ``None``: no levelling, today's output to the bit.
    ``loudness_groups``: one hashable per utterance; the utterances of a group (the sentences of one document) are measured as one
    programme and share ONE gain, whichever buckets they fall into — the buckets' block energies and peaks stay on the device until the
    last bucket has run, then one gating launch and one multiply per bucket follow (ungrouped calls keep the overlap of a bucket's copy
    with the next bucket's kernels).  ``return_levels``: ``(audio, levels)`` with one dict per utterance — ``lufs`` (measured, of its
    group), ``gain_db`` and ``gain`` (the fp32 factor that was applied), ``peak`` (its own sample peak before the gain), ``limited``,
    ``silent``.  ``peak="true"``: ``peak_ceiling_db`` is in dBTP — the gain is lowered where the TRUE peak (``audio.true_peak``, measured
    on the device at the output rate) of the utterance, or of its group, would pass the ceiling; the levels then carry ``true_peak``
    beside ``peak``.  ``"sample"`` is today's output to the bit; ``"true"`` without ``target_lufs`` raises.
    ``limiter=True``: the target holds (``audio.normalize_loudness(limiter=True)``, on both paths): the gain goes to the target without
    the ceiling and the look-ahead limiter keeps ``peak_ceiling_db`` as a TRUE-peak ceiling, ``lookahead_ms`` / ``release_ms`` /
    ``makeup_passes`` as there; it runs after the resampling, before the one copy.  ``peak=`` then only selects what the levels report;
    they gain ``lufs_out`` (the loudness of what is returned, of the utterance's group) and ``min_gain_db`` (its own deepest gain
    reduction), and ``limited`` means "the limiter engaged on its group".  A grouped call limits behind the last bucket, on the caller's
    stream.  ``False`` is today's output to the bit; ``True`` without ``target_lufs`` raises."""
    if model.device.type != "cuda":
        raise RuntimeError("bert_vits2_amd.serving needs the model on a GPU: there is no CPU fallback")
    if noise is not None and any(u.seed is not None for u in utts):
        raise ValueError("noise= (injected tensors) and Utterance(seed=...) exclude each other")
    dev = model.device
    hop = model.hp.total_upsample
    output_rate = _output_rate(model, output_rate)
    if output_rate is not None:
        hop = 1                                            # the buckets' lengths then count output-rate samples
    level = _level_plan(model, utts, output_rate, target_lufs, peak_ceiling_db, loudness_groups, return_levels, peak,
                        dict(lookahead_ms=lookahead_ms, release_ms=release_ms, makeup_passes=makeup_passes) if limiter else None)
    results: List[Optional[np.ndarray]] = [None] * len(utts)
    pending = []
    lanes = replicas(model, requests_in_flight) if requests_in_flight > 1 else [(model, None)]
    call = dict(sdp_ratio=sdp_ratio, noise_scale=noise_scale, noise_scale_w=noise_scale_w, length_scale=length_scale)
    per_item = any(getattr(u, k) is not None for u in utts for k in call)
    gvec = speaker_vectors(model, utts)                    # reference spectrograms are encoded here, once per distinct object
    if requests_in_flight > 1:
        torch.cuda.current_stream(dev).synchronize()       # inputs prepared on the caller's stream are visible to the lanes
    weights = None
    if per_item and any(u.length_scale is not None for u in utts):
        weights = [float(length_scale if u.length_scale is None else u.length_scale) for u in utts]
    for bi, idx in enumerate(plan_batches([u.length for u in utts], max_batch, max_pad_ratio, weights)):
        lane, lane_stream = lanes[bi % len(lanes)]
        if per_item:                                        # one value per batch item: [B] tensors (models.item_control)
            ctl = {k: torch.tensor([float(v if getattr(utts[i], k) is None else getattr(utts[i], k)) for i in idx],
                                   dtype=torch.float32) for k, v in call.items()}
        else:
            ctl = call
        with torch.cuda.stream(lane_stream) if lane_stream is not None else contextlib.nullcontext():
            _run_bucket(lane, utts, idx, dev, noise, pending, as_pcm16, gvec, output_rate=output_rate, level=level, **ctl)
    if level is not None and level["ids"] is not None:
        _level_groups(level, pending, as_pcm16, dev)
    levels: List[Optional[dict]] = [None] * len(utts)
    for idx, host, y_len, ev, *lv in pending:
        ev.synchronize()
        for r, i in enumerate(idx):
            results[i] = host[r, :int(y_len[r]) * hop].numpy().copy()
            if lv:
                lufs, gain, pk, flags = (float(v) for v in lv[0][:4, r])
                levels[i] = dict(lufs=lufs, gain_db=20.0 * math.log10(gain), gain=gain, peak=pk, limited=bool(int(flags) & 2),
                                 silent=bool(int(flags) & 1))
                if level["limiter"] is not None:               # the last two rows
                    levels[i].update(lufs_out=float(lv[0][-2, r]), min_gain_db=float(lv[0][-1, r]))
                if level["true"]:
                    levels[i]["true_peak"] = float(lv[0][4, r])
    return (results, levels) if return_levels else results


DOCUMENT_LEVELS = ("piece", "paragraph", "document")


def document_timeline(documents, rate: int, *, interval_between_sent=0.2, interval_between_para=1.0, cut_by_sent=True):
    """The timeline of reference webui.py ``tts_split`` for ``documents`` (a document: a list of paragraphs; a paragraph: a list of
    sentences; a sentence: an ``Utterance`` or a list of them, joined with no pause between).  Returns ``(utts, timeline)``: the pieces in
    reading order and, per document, a list of ``("piece", index into utts, paragraph number over the whole call)`` / ``("silence",
    samples)``.  With ``cut_by_sent`` ``int(rate * interval_between_sent)`` samples follow every sentence and ``int(rate *
    (interval_between_para - interval_between_sent))`` more a paragraph's last, where that difference is positive; without it a paragraph's
    pieces follow each other directly and ``int(rate * interval_between_para)`` samples follow the paragraph.  The pause behind the last
    paragraph is kept, as the reference keeps it."""
    from . import audio
    for v in (interval_between_sent, interval_between_para):
        if not (math.isfinite(float(v)) and float(v) >= 0):
            raise ValueError("interval_between_sent and interval_between_para must be finite and not negative")
    sent = audio.pause_samples(rate, interval_between_sent)
    extra = audio.paragraph_pause_samples(rate, interval_between_para, interval_between_sent)
    para_only = audio.pause_samples(rate, interval_between_para)
    utts, timeline, n_para = [], [], 0
    if isinstance(documents, Utterance) or len(documents) < 1:
        raise ValueError("documents must be a non-empty list of documents (lists of paragraphs)")
    for d, doc in enumerate(documents):
        if isinstance(doc, Utterance) or len(doc) < 1:
            raise ValueError(f"document {d} must be a non-empty list of paragraphs")
        line = []
        for p, para in enumerate(doc):
            if isinstance(para, Utterance) or len(para) < 1:
                raise ValueError(f"document {d}, paragraph {p} must be a non-empty list of sentences")
            for s, sentence in enumerate(para):
                pieces = [sentence] if isinstance(sentence, Utterance) else list(sentence)
                if not pieces or not all(isinstance(u, Utterance) for u in pieces):
                    raise ValueError(f"document {d}, paragraph {p}, sentence {s} must be an Utterance or a non-empty list of them")
                for u in pieces:
                    line.append(("piece", len(utts), n_para))
                    utts.append(u)
                if cut_by_sent:
                    line.append(("silence", sent))
            if not cut_by_sent:
                line.append(("silence", para_only))
            elif extra > 0:
                line.append(("silence", extra))
            n_para += 1
        timeline.append(line)
    return utts, timeline


@torch.no_grad()
def synthesize_documents(model, documents, *, interval_between_sent: float = 0.2, interval_between_para: float = 1.0,
                         cut_by_sent: bool = True, level: str = "piece", target_lufs: Optional[float] = None,
                         peak_ceiling_db: float = -1.0, as_pcm16: bool = True, output_rate: Optional[int] = None,
                         return_offsets: bool = False, peak: str = "sample", sdp_ratio=0.5, noise_scale=0.6, noise_scale_w=0.9,
                         length_scale=1.0,
                         max_batch: int = 32, max_pad_ratio: float = 1.25, noise: Optional[Sequence] = None,
                         requests_in_flight: int = 1):
    """Whole documents: what the reference's web UI does behind synthesis (webui.py ``tts_split`` / ``generate_audio``) on the device —
    every piece levelled, a pause behind every sentence, a longer one behind every paragraph, everything joined — and ONE copy out per
    document.  ``documents``: see ``document_timeline``; the defaults are the reference web UI's sliders (webui.py:477-490), pauses are
    ``int(rate * seconds)`` at the output rate.  All pieces of all documents share the length buckets of ``synthesize`` (same kwargs:
    controls, voices, seeds, ``output_rate``, ``requests_in_flight``); the waves and their lengths stay on the device, one
    ``audio.assemble`` lays the documents out there (the lengths never reach the host before it), then the host reads the totals and the
    offsets in one small copy and exactly ``totals[d]`` samples per document into pinned memory.
    ``level``: ``"piece"`` — each piece under its own peak, ``(x / max|x|) * 32767`` truncated, the reference's document bit for bit
    (``synthesize(as_pcm16=True)`` joined with zero pauses); ``"paragraph"`` / ``"document"`` — under the peak of its paragraph / document,
    which keeps the level differences inside it.  ``target_lufs``: every document is measured as one programme (``synthesize``'s
    ``loudness_groups``) and leaves at that loudness under ``peak_ceiling_db``: one gain per document, the fixed-gain 16-bit form; it
    overrides ``level``; ``peak="true"`` puts the ceiling in dBTP (the document's true peak, ``synthesize``'s ``peak``).
    ``as_pcm16=False``: fp32 (``x / peak``, or ``x * gain``).
    Returns one 1-D array per document; with ``return_offsets`` ``(audio, offsets)``, ``offsets[d]`` a list of ``(start sample, length)``
    per piece of document d in reading order — for subtitles and highlighting."""
    from . import audio
    if model.device.type != "cuda":
        raise RuntimeError("bert_vits2_amd.serving needs the model on a GPU: there is no CPU fallback")
    if level not in DOCUMENT_LEVELS:
        raise ValueError(f"level must be one of {DOCUMENT_LEVELS}, got {level!r}")
    dev = model.device
    output_rate = _output_rate(model, output_rate)
    rate = int(output_rate if output_rate is not None else model.hp.sampling_rate)
    utts, timeline = document_timeline(documents, rate, interval_between_sent=interval_between_sent,
                                       interval_between_para=interval_between_para, cut_by_sent=cut_by_sent)
    if noise is not None and any(u.seed is not None for u in utts):
        raise ValueError("noise= (injected tensors) and Utterance(seed=...) exclude each other")
    doc_of = [d for d, line in enumerate(timeline) for e in line if e[0] == "piece"]
    loud = _level_plan(model, utts, output_rate, target_lufs, peak_ceiling_db, doc_of if target_lufs is not None else None, False, peak)
    hop = model.hp.total_upsample if output_rate is None else 1
    lanes = replicas(model, requests_in_flight) if requests_in_flight > 1 else [(model, None)]
    call = dict(sdp_ratio=sdp_ratio, noise_scale=noise_scale, noise_scale_w=noise_scale_w, length_scale=length_scale)
    per_item = any(getattr(u, k) is not None for u in utts for k in call)
    gvec = speaker_vectors(model, utts)
    if requests_in_flight > 1:
        torch.cuda.current_stream(dev).synchronize()       # inputs prepared on the caller's stream are visible to the lanes
    weights = None
    if per_item and any(u.length_scale is not None for u in utts):
        weights = [float(length_scale if u.length_scale is None else u.length_scale) for u in utts]
    sources, lengths, where, events = [], [], {}, []
    for bi, idx in enumerate(plan_batches([u.length for u in utts], max_batch, max_pad_ratio, weights)):
        lane, lane_stream = lanes[bi % len(lanes)]
        if per_item:
            ctl = {k: torch.tensor([float(v if getattr(utts[i], k) is None else getattr(utts[i], k)) for i in idx],
                                   dtype=torch.float32) for k, v in call.items()}
        else:
            ctl = call
        with torch.cuda.stream(lane_stream) if lane_stream is not None else contextlib.nullcontext():
            wave, y_len, lens = _bucket_wave(lane, utts, idx, dev, noise, gvec, output_rate, **ctl)
            if loud is not None:
                _hold_levels(loud, idx, wave, y_len * hop if lens is None else lens, y_len, dev)    # with the event _gate_held waits for
            elif lane_stream is not None:
                ev = torch.cuda.Event()
                ev.record()
                events.append(ev)
        for r, i in enumerate(idx):
            where[i] = (len(sources), r)
        sources.append(wave)
        lengths.append((y_len.contiguous(), hop))
    main = torch.cuda.current_stream(dev)
    gain = None
    if loud is not None:
        gain = _gate_held(loud, dev)[0]["gain"]             # one gain per document, on the caller's stream behind every bucket
        mode = "gain"
    else:
        for ev in events:
            main.wait_event(ev)
        mode = "piece" if level == "piece" else "group"
    segments, pieces = [], []
    for d, line in enumerate(timeline):
        rows = []
        for e in line:
            if e[0] == "piece":
                k, r = where[e[1]]
                group = d if (mode == "gain" or level == "document") else (e[2] if level == "paragraph" else 0)
                rows.append(len(segments))
                segments.append(audio.Piece(k, r, group, d))
            else:
                segments.append(audio.Silence(e[1], d))
        pieces.append(rows)
    buffers, offsets, totals = audio.assemble(sources, lengths, segments, level=mode, gain=gain, as_pcm16=as_pcm16)
    n_docs = len(timeline)
    small = torch.cat([totals, offsets])
    host_small = torch.empty(small.shape, dtype=torch.int64, pin_memory=True)
    host_small.copy_(small, non_blocking=True)
    main.synchronize()                                     # the layout is known (and the audio written): now the host can size its copies
    tot = [int(v) for v in host_small[:n_docs]]
    off = [int(v) for v in host_small[n_docs:]]
    hosts = []
    for d in range(n_docs):
        host = torch.empty(tot[d], dtype=buffers[d].dtype, pin_memory=True)
        host.copy_(buffers[d][:tot[d]], non_blocking=True)
        hosts.append(host)
    main.synchronize()
    results = [h.numpy().copy() for h in hosts]
    if not return_offsets:
        return results
    ends = [[(off[s + 1] if s + 1 < len(off) and segments[s + 1].doc == d else tot[d]) for s in rows] for d, rows in enumerate(pieces)]
    return results, [[(off[s], e - off[s]) for s, e in zip(rows, ends[d])] for d, rows in enumerate(pieces)]


def _level_plan(model, utts, output_rate, target_lufs, peak_ceiling_db, loudness_groups, return_levels, peak="sample",
                limiter: Optional[dict] = None) -> Optional[dict]:
    """The loudness arguments of ``synthesize``, checked before any work: ``None`` without a target."""
    from . import audio
    if peak not in audio.PEAKS:
        raise ValueError(f"peak must be one of {audio.PEAKS}, got {peak!r}")
    if target_lufs is None:
        if loudness_groups is not None or return_levels:
            raise ValueError("loudness_groups and return_levels need target_lufs")
        if peak != "sample":
            raise ValueError("peak='true' needs target_lufs")
        if limiter is not None:
            raise ValueError("limiter=True needs target_lufs")
        return None
    if not (math.isfinite(float(target_lufs)) and math.isfinite(float(peak_ceiling_db))):
        raise ValueError("target_lufs and peak_ceiling_db must be finite")
    rate = int(output_rate if output_rate is not None else model.hp.sampling_rate)
    audio.loudness_plan(rate)                               # ValueError naming the envelope
    if limiter is not None:
        audio._limiter_args(rate, 1, **limiter)
    ids = None
    if loudness_groups is not None:
        keys = list(loudness_groups)
        if len(keys) != len(utts):
            raise ValueError("loudness_groups takes one hashable per utterance")
        dense = {}
        ids = [dense.setdefault(k, len(dense)) for k in keys]
    return dict(rate=rate, target=float(target_lufs), ceiling=float(peak_ceiling_db), ids=ids, held=[], true=peak == "true",
                limiter=limiter)


def _gate_held(level, dev):
    """Groups that span buckets: every bucket has left its audio, block mean squares and peaks on the device (``level["held"]``).  One
    gating launch over all of them on the caller's stream, ordered behind every bucket by its event.  Returns the gate's outputs and the
    group id of every held row, bucket after bucket."""
    from . import audio
    held = level["held"]
    main = torch.cuda.current_stream(dev)
    for h in held:
        main.wait_event(h["ev"])
    width = max(h["block_ms"].shape[1] for h in held)
    S = max(h["wave"].shape[1] for h in held)
    ms = torch.cat([torch.nn.functional.pad(h["block_ms"], (0, width - h["block_ms"].shape[1])) for h in held])
    rows = [i for h in held for i in h["idx"]]
    groups = torch.tensor([level["ids"][i] for i in rows], dtype=torch.int32).to(dev)
    n_groups = max(level["ids"]) + 1
    which = "true_peak" if level["true"] else "peak"         # what the ceiling limits
    ceiling = level["ceiling"] if level["limiter"] is None else audio.NO_CEILING_DB      # the limiter keeps the ceiling instead
    m = audio.loudness_gate(ms, torch.cat([h["lens"] for h in held]), S, torch.cat([h[which] for h in held]), level["rate"], groups,
                            n_groups, level["target"], ceiling)
    return m, groups


def _level_groups(level, pending, as_pcm16, dev):
    """``_gate_held``; then, on each bucket's own stream and behind the gate's event, one multiply and the bucket's copy."""
    from . import audio
    held = level["held"]
    main = torch.cuda.current_stream(dev)
    m, groups = _gate_held(level, dev)
    if level["limiter"] is not None:
        return _limit_groups(level, pending, as_pcm16, dev, m, groups)
    gated = torch.cuda.Event()
    gated.record(main)
    o = 0
    for h in held:
        B = len(h["idx"])
        g = groups[o:o + B]
        with torch.cuda.stream(h["stream"]) if h["stream"] is not None else contextlib.nullcontext():
            torch.cuda.current_stream(dev).wait_event(gated)
            out = audio.loudness_apply(h["wave"], h["lens"], level["rate"], m["gain"], g, as_pcm16)
            gl = g.long()
            lv = [m["lufs"][gl], m["gain"][gl].double(), h["peak"].double(), m["flags"][gl].double()]
            if level["true"]:
                lv.append(h["true_peak"].double())
            _enqueue_copy(pending, h["idx"], out, h["y_len"], torch.stack(lv))
        o += B


def _limit_groups(level, pending, as_pcm16, dev, m, groups):
    """The limiter under a grouped target (``audio.limit_to_target`` over buckets), on the caller's stream behind ``_gate_held``: every
    bucket is limited under its groups' gains; the outputs' block energies go through one gate, which gives every group its loudness;
    ``makeup_passes`` times the gains are raised by what is missing and the buckets are limited again from their unlevelled audio."""
    from . import audio
    held, lim, rate = level["held"], level["limiter"], level["rate"]
    n_groups = m["gain"].numel()
    spans, o = [], 0
    for h in held:
        spans.append(groups[o:o + len(h["idx"])])
        o += len(h["idx"])
    S = max(h["wave"].shape[1] for h in held)
    lens = torch.cat([h["lens"] for h in held])
    gain = m["gain"]
    for left in range(int(lim["makeup_passes"]), -1, -1):
        outs = [audio.limit_apply(h["wave"], h["lens"], rate, gain, g, level["ceiling"], lim["lookahead_ms"], lim["release_ms"],
                                  as_pcm16 and left == 0) for h, g in zip(held, spans)]
        ms = [audio.loudness_measure(r["out"], h["lens"], rate, gate=False) for r, h in zip(outs, held)]
        width = max(v["block_ms"].shape[1] for v in ms)
        lufs_out = audio.loudness_gate(torch.cat([torch.nn.functional.pad(v["block_ms"], (0, width - v["block_ms"].shape[1])) for v in ms]),
                                       lens, S, torch.cat([v["peak"] for v in ms]), rate, groups, n_groups)["lufs"]
        if left:
            up = torch.pow(10.0, (level["target"] - lufs_out) / 20.0)
            gain = torch.where(torch.isfinite(up), gain.to(torch.float64) * up, gain.to(torch.float64)).to(torch.float32)
    hit = torch.zeros(n_groups, dtype=torch.int64, device=dev).index_add_(
        0, groups.long(), (torch.cat([r["limited_samples"] for r in outs]) > 0).to(torch.int64)) > 0
    flags = (m["flags"] & 1) + 2 * hit.to(torch.int32)
    for h, g, r in zip(held, spans, outs):
        gl = g.long()
        lv = [m["lufs"][gl], gain[gl].double(), h["peak"].double(), flags[gl].double()]
        if level["true"]:
            lv.append(h["true_peak"].double())
        lv += [lufs_out[gl], audio.min_gain_db(r["min_gain"])]
        _enqueue_copy(pending, h["idx"], r["out"], h["y_len"], torch.stack(lv))


def _enqueue_copy(pending, idx, audio, y_len, levels=None):
    """One async D2H per bucket into pinned memory (audio AND lengths, levels if any): nothing here blocks the host, so the next bucket's
    kernels are enqueued while this copy runs; the drain loop of ``synthesize`` waits on the bucket's event."""
    host = torch.empty(audio.shape, dtype=audio.dtype, pin_memory=True)
    host.copy_(audio, non_blocking=True)
    host_len = torch.empty(y_len.shape, dtype=torch.int64, pin_memory=True)
    host_len.copy_(y_len, non_blocking=True)
    extra = []
    if levels is not None:
        host_lv = torch.empty(levels.shape, dtype=torch.float64, pin_memory=True)
        host_lv.copy_(levels, non_blocking=True)
        extra.append(host_lv)
    ev = torch.cuda.Event()
    ev.record()
    pending.append((idx, host, host_len, ev, *extra))


def _output_rate(model, output_rate) -> Optional[int]:
    """``None`` where the audio stays at the model's rate; else the rate, checked against the resampler's envelope before any work."""
    if output_rate is None or int(output_rate) == int(model.hp.sampling_rate):
        return None
    from . import audio
    audio.resample_plan(int(model.hp.sampling_rate), int(output_rate))
    return int(output_rate)


def _bucket_wave(model, utts, idx, dev, noise, gvec, output_rate, sdp_ratio, noise_scale, noise_scale_w, length_scale):
    """One bucket's audio on the CURRENT stream, left on the device: collate, infer (exact lengths), optional resampling.  Returns ``(wave
    [B, S], y_len, lens)``: ``y_len`` counts frames, or samples after a resampling; ``lens`` counts samples (``None`` at the model's rate:
    ``y_len * hop``)."""
    batch, kw = _bucket_inputs(model, utts, idx, dev, noise, gvec)
    o, _attn, y_mask, _ = model.infer(batch["x"], batch["x_lengths"], batch["sid"], batch["tone"], batch["language"],
                                      batch["bert"], batch["ja_bert"], batch["en_bert"], sdp_ratio=sdp_ratio,
                                      noise_scale=noise_scale, noise_scale_w=noise_scale_w, length_scale=length_scale,
                                      want_attn=False, exact_lengths=True, **kw)
    y_len = model.last_encode["y_lengths"]             # int64 [B], already on the device (phase A output)
    if output_rate is None:
        return o[:, 0], y_len, None
    from . import audio as _audio
    wave, y_len = _audio.resample(o[:, 0], y_len * model.hp.total_upsample, model.hp.sampling_rate, output_rate)
    return wave, y_len, y_len


def _run_bucket(model, utts, idx, dev, noise, pending, as_pcm16, gvec, sdp_ratio, noise_scale, noise_scale_w, length_scale,
                output_rate=None, level=None):
    """One bucket on the CURRENT stream: ``_bucket_wave``, optional levelling or PCM16, async D2H into pinned memory.  The lengths that
    travel with it count frames, or samples after a resampling."""
    wave, y_len, lens = _bucket_wave(model, utts, idx, dev, noise, gvec, output_rate, sdp_ratio, noise_scale, noise_scale_w, length_scale)
    from . import audio as _audio
    if lens is None and level is not None:
        lens = y_len * model.hp.total_upsample
    if level is None:
        audio = pcm16(model, wave[:, None], y_len, hop=None if output_rate is None else 1) if as_pcm16 else wave
        _enqueue_copy(pending, idx, audio, y_len)
    elif level["ids"] is None and level["limiter"] is not None:   # the gain to the target alone; the limiter keeps the ceiling
        B = wave.shape[0]
        lim = level["limiter"]
        m0 = _audio.loudness_measure(wave, lens, level["rate"], gate=False)
        m = _audio.loudness_gate(m0["block_ms"], lens, wave.shape[1], m0["peak"], level["rate"], None, B, level["target"], _audio.NO_CEILING_DB)
        audio, r = _audio.limit_to_target(wave, lens, level["rate"], m["gain"], None, B, level["target"], level["ceiling"],
                                          lim["lookahead_ms"], lim["release_ms"], lim["makeup_passes"], as_pcm16)
        lv = [m["lufs"], r["gain"].double(), m0["peak"].double(), ((m["flags"] & 1) + 2 * r["limited"].to(torch.int32)).double()]
        if level["true"]:
            lv.append(_audio.true_peak_measure(wave, lens, level["rate"]).double())
        _enqueue_copy(pending, idx, audio, y_len, torch.stack(lv + [r["lufs_out"], r["min_gain_db"]]))
    elif level["ids"] is None and level["true"]:       # the same, under a true-peak ceiling: blocks and sample peaks, true peaks, the gate
        m0 = _audio.loudness_measure(wave, lens, level["rate"], gate=False)
        tp = _audio.true_peak_measure(wave, lens, level["rate"])
        m = _audio.loudness_gate(m0["block_ms"], lens, wave.shape[1], tp, level["rate"], None, wave.shape[0], level["target"], level["ceiling"])
        audio = _audio.loudness_apply(wave, lens, level["rate"], m["gain"], None, as_pcm16)
        _enqueue_copy(pending, idx, audio, y_len,
                      torch.stack([m["lufs"], m["gain"].double(), m0["peak"].double(), m["flags"].double(), tp.double()]))
    elif level["ids"] is None:                         # every utterance its own programme: measure, scale, copy
        m = _audio.loudness_measure(wave, lens, level["rate"], None, None, level["target"], level["ceiling"])
        audio = _audio.loudness_apply(wave, lens, level["rate"], m["gain"], None, as_pcm16)
        _enqueue_copy(pending, idx, audio, y_len, torch.stack([m["lufs"], m["gain"].double(), m["peak"].double(), m["flags"].double()]))
    else:                                              # groups may span buckets: energies and peaks wait on the device (_level_groups)
        _hold_levels(level, idx, wave, lens, y_len, dev)


def _hold_levels(level, idx, wave, lens, y_len, dev):
    """A bucket of a grouped measurement: its block energies and peaks (the true peaks beside the sample peaks where the ceiling is in
    dBTP), and an event behind them, in ``level["held"]``."""
    from . import audio as _audio
    m = _audio.loudness_measure(wave, lens, level["rate"], gate=False)
    tp = _audio.true_peak_measure(wave, lens, level["rate"]) if level["true"] else None
    ev = torch.cuda.Event()
    ev.record()
    level["held"].append(dict(idx=idx, wave=wave, lens=lens, y_len=y_len, block_ms=m["block_ms"], peak=m["peak"], true_peak=tp, ev=ev,
                              stream=torch.cuda.current_stream(dev)))


def _bucket_inputs(model, utts, idx, dev, noise, gvec):
    """The collated batch of one bucket and the keyword extras of its ``infer`` call (speaker vectors, injected noise)."""
    group = [utts[i] for i in idx]
    batch = collate(group, dev)
    kw = {}
    if any(gvec[i] is not None for i in idx):
        # a bucket that mixes voices by vector and by index runs on ONE [B, gin]: the table rows of the sid utterances are fetched on
        # the device (bit-identical to the lookup inside phase A, which reads the same row through the same code)
        rows = model.stage_emb_g(batch["sid"]) if any(gvec[i] is None for i in idx) else None
        kw["g"] = torch.stack([rows[r] if gvec[i] is None else gvec[i] for r, i in enumerate(idx)])
    if any(utts[i].seed is not None for i in idx):
        # a bucket with a seeded utterance runs the seeded path; the others get a seed from torch's CPU generator (torch.manual_seed governs them)
        if noise is not None:
            raise ValueError("noise= (injected tensors) and Utterance(seed=...) exclude each other")
        kw["seeds"] = torch.tensor([utts[i].seed if utts[i].seed is not None else
                                    int(torch.randint(-2 ** 63, 2 ** 63 - 1, (1,), dtype=torch.int64)) for i in idx], dtype=torch.int64)
    if noise is not None:
        T = batch["x"].shape[1]
        Tz = max(int(noise[i][1].shape[1]) for i in idx)
        nw = torch.zeros(len(idx), 2, T)
        nz = torch.zeros(len(idx), model.hp.inter_channels, Tz)
        for r, i in enumerate(idx):
            nw[r, :, :noise[i][0].shape[1]] = noise[i][0]
            nz[r, :, :noise[i][1].shape[1]] = noise[i][1]
        kw.update(noise_w=nw.to(dev), noise_z=nz.to(dev))
    if any(utts[i].durations is not None for i in idx):
        # given durations take the place of the predicted ones after phase A; a bucket may mix both kinds of utterance
        wc = torch.zeros(len(idx), batch["x"].shape[1])
        for r, i in enumerate(idx):
            if utts[i].durations is not None:
                wc[r, :utts[i].length] = utts[i].durations
        kw["w_ceil"] = wc.to(dev)
        if any(utts[i].durations is None for i in idx):
            kw["w_ceil_items"] = torch.tensor([utts[i].durations is not None for i in idx])
    return batch, kw


def synthesize_stream(model, utts: Sequence[Utterance], *, sdp_ratio=0.5, noise_scale=0.6, noise_scale_w=0.9, length_scale=1.0,
                      max_batch: int = 32, max_pad_ratio: float = 1.25, chunk_frames: int = 64,
                      first_chunk_frames: Optional[int] = None, as_pcm16: bool = False, noise: Optional[Sequence] = None,
                      output_rate: Optional[int] = None):
    """``synthesize`` with the audio handed out as it is produced: a generator of ``(utterance_index, start_sample, np.ndarray)``.  Same
    buckets, per-utterance controls, voices and ``exact_lengths=True`` as ``synthesize``; each bucket runs ``infer_stream`` and its
    Generator chunk by chunk (``chunk_frames`` kept frames, ``first_chunk_frames`` for the first).  A bucket has two pinned host buffers:
    chunk n + 1 is enqueued before the host waits on chunk n's copy event, so the device-to-host copy of a chunk runs under the next
    chunk's Generator.  An utterance's pieces arrive in order with contiguous offsets, and nothing is yielded past its own length.
    ``as_pcm16``: int16 pieces, ``trunc(x * 32767)`` — a FIXED gain, unlike ``synthesize``'s per-utterance peak normalisation (a stream
    cannot know the peak; the two differ by exactly the factor 1 / max|x| of the utterance).
    ``output_rate``: the pieces leave at that sampling rate (``infer_stream(output_rate=...)``: resampled on the device chunk by chunk,
    PCM after the resampling); offsets and lengths then count output-rate samples."""
    if model.device.type != "cuda":
        raise RuntimeError("bert_vits2_amd.serving needs the model on a GPU: there is no CPU fallback")
    if noise is not None and any(u.seed is not None for u in utts):
        raise ValueError("noise= (injected tensors) and Utterance(seed=...) exclude each other")
    dev = model.device
    hop = model.hp.total_upsample
    output_rate = _output_rate(model, output_rate)
    call = dict(sdp_ratio=sdp_ratio, noise_scale=noise_scale, noise_scale_w=noise_scale_w, length_scale=length_scale)
    per_item = any(getattr(u, k) is not None for u in utts for k in call)
    gvec = speaker_vectors(model, utts)
    weights = None
    if per_item and any(u.length_scale is not None for u in utts):
        weights = [float(length_scale if u.length_scale is None else u.length_scale) for u in utts]
    for idx in plan_batches([u.length for u in utts], max_batch, max_pad_ratio, weights):
        if per_item:
            ctl = {k: torch.tensor([float(v if getattr(utts[i], k) is None else getattr(utts[i], k)) for i in idx],
                                   dtype=torch.float32) for k, v in call.items()}
        else:
            ctl = call
        batch, kw = _bucket_inputs(model, utts, idx, dev, noise, gvec)
        st = model.infer_stream(batch["x"], batch["x_lengths"], batch["sid"], batch["tone"], batch["language"], batch["bert"],
                                batch["ja_bert"], batch["en_bert"], want_attn=False, exact_lengths=True, chunk_frames=chunk_frames,
                                first_chunk_frames=first_chunk_frames, as_pcm16=as_pcm16, output_rate=output_rate, **ctl, **kw)
        ends = [n * hop for n in st.y_lengths_host]
        if output_rate is not None:
            from . import audio
            ends = [audio.resample_length(model.hp.sampling_rate, output_rate, e) for e in ends]
        width = st.max_chunk_samples
        hosts = [torch.empty(len(idx), width, dtype=torch.int16 if as_pcm16 else torch.float32, pin_memory=True) for _ in range(2)]

        def pieces(start, n, host, ev):
            ev.synchronize()
            for r, i in enumerate(idx):
                keep = min(n, ends[r] - start)
                if keep > 0:
                    yield i, start, host[r, :keep].numpy().copy()

        waiting = None
        for k, (start, audio) in enumerate(st):
            host = hosts[k & 1]                                 # chunk k - 2 used it and was drained before chunk k - 1 was enqueued
            n = audio.shape[1]
            host[:, :n].copy_(audio, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
            if waiting is not None:
                yield from pieces(*waiting)
            waiting = (start, n, host, ev)
        if waiting is not None:
            yield from pieces(*waiting)


@torch.no_grad()
def align(model, utts: Sequence[Utterance], specs: Optional[Sequence[torch.Tensor]] = None, *,
          latents: Optional[Sequence[torch.Tensor]] = None, max_batch: int = 32, max_pad_ratio: float = 1.25) -> List[np.ndarray]:
    """Frames per phone of each utterance's recording.  ``specs[i]`` is the recording's linear spectrogram ``[spec_channels, Ty_i]``
    (``reference_spectrogram(model, wav)``); it goes through the posterior encoder (``model.load_posterior`` first; deterministic,
    ``z = m_q``) and the forward flow.  Alternatively ``latents[i]`` ``[inter, Ty_i]`` is the recording's latent already in the prior's
    space.  Utterances are bucketed by length like ``synthesize``; a bucket is ONE ragged batch through phase A (the text's prior), the
    recording's side, ``align.neg_cent`` and ``align.maximum_path``.  Returns one int64 array ``[T_i]`` per utterance, in input order,
    ready for ``Utterance(durations=...)``."""
    from . import align as _align
    from . import models as _models
    if model.device.type != "cuda":
        raise RuntimeError("bert_vits2_amd.serving needs the model on a GPU: there is no CPU fallback")
    if (specs is None) == (latents is None):
        raise ValueError("serving.align takes specs or latents=, exactly one of them")
    from_spec = specs is not None
    if from_spec:
        model._need_posterior("serving.align")
    latents = specs if from_spec else latents
    if len(latents) != len(utts):
        raise ValueError("one recording per utterance")
    dev, Ci = model.device, (model.hp.spec_channels if from_spec else model.hp.inter_channels)
    for i, (u, z) in enumerate(zip(utts, latents)):
        if z.dim() != 2 or z.shape[0] != Ci:
            raise ValueError(f"utterance {i}: the {'spectrogram' if from_spec else 'latent'} must be [{Ci}, Ty], got {tuple(z.shape)}")
        if u.length > z.shape[1]:
            raise ValueError(f"utterance {i}: {u.length} phones cannot be aligned to {z.shape[1]} frames")
    gvec = speaker_vectors(model, utts)
    results: List[Optional[np.ndarray]] = [None] * len(utts)
    for idx in plan_batches([u.length for u in utts], max_batch, max_pad_ratio):
        batch, kw = _bucket_inputs(model, utts, idx, dev, None, gvec)
        B, T = batch["x"].shape
        # the prior does not depend on the duration predictors: sdp_ratio 0 runs the deterministic one only, and its noise is not read
        seeds = kw.get("seeds")                     # a seeded bucket: the posterior is SAMPLED from each utterance's seed (else z = m_q)
        enc = model.encode_durations(batch["x"], batch["x_lengths"], batch["sid"], batch["tone"], batch["language"], batch["bert"],
                                     batch["ja_bert"], batch["en_bert"], None if seeds is not None else _models.draw_noise_w(B, T, None),
                                     sdp_ratio=0.0, lean=True, g=kw.get("g"), seeds=seeds)
        y_len = [int(latents[i].shape[1]) for i in idx]
        z_p = torch.zeros(B, Ci, max(y_len), dtype=torch.float32, device=dev)
        for r, i in enumerate(idx):
            z_p[r, :, :y_len[r]] = latents[i].to(dev, torch.float32)
        if from_spec:
            yl = torch.tensor(y_len, dtype=torch.int64)
            z_p = model.stage_flow_forward(model.posterior_encode(z_p, yl, g=enc["g"], seeds=seeds)["z"], yl, enc["g"])
        out = _align.align_latent(enc, z_p, y_len, x_lengths=[utts[i].length for i in idx])
        dur = out["durations"].cpu().numpy()
        for r, i in enumerate(idx):
            results[i] = dur[r, :utts[i].length].copy()
    return results


@torch.no_grad()
def score(model, utts: Sequence[Utterance], specs: Sequence[torch.Tensor], *, use_durations: bool = False, max_batch: int = 32,
          max_pad_ratio: float = 1.25) -> List[dict]:
    """How well the model explains each utterance's recording (``SynthesizerTrn.score``; ``model.load_posterior`` and
    ``model.load_sdp_forward`` first).  ``specs[i]`` is the recording's linear spectrogram ``[spec_channels, Ty_i]``.  Utterances are
    bucketed by length like ``align``; a bucket is ONE ragged batch.  ``use_durations``: every utterance carries ``durations`` and is
    scored with them (a timing transfer judged before it is spoken) instead of being aligned.  ``Utterance(seed=...)`` fixes the
    utterance's three draws, so its numbers do not depend on the bucket it lands in; unseeded utterances draw from torch's CPU generator.
    Returns one dict of numpy arrays per utterance, in input order, cut to the utterance's own ``T`` and ``T_y``: ``nll`` (scalar),
    ``nll_sym`` [T], ``kl`` (scalar), ``kl_frame`` [Ty], ``durations`` [T], ``score`` (the aligner's, absent with ``use_durations``),
    ``l_length_dp`` and ``l_length_sdp_mse``."""
    if model.device.type != "cuda":
        raise RuntimeError("bert_vits2_amd.serving needs the model on a GPU: there is no CPU fallback")
    model._need_posterior("serving.score")
    model._need_sdp_forward("serving.score")
    if len(specs) != len(utts):
        raise ValueError("one recording per utterance")
    dev, S = model.device, model.hp.spec_channels
    for i, (u, y) in enumerate(zip(utts, specs)):
        if y.dim() != 2 or y.shape[0] != S:
            raise ValueError(f"utterance {i}: the spectrogram must be [{S}, Ty], got {tuple(y.shape)}")
        if u.length > y.shape[1]:
            raise ValueError(f"utterance {i}: {u.length} phones cannot be aligned to {y.shape[1]} frames")
        if use_durations and u.durations is None:
            raise ValueError(f"utterance {i}: use_durations needs Utterance(durations=...)")
    gvec = speaker_vectors(model, utts)
    results: List[Optional[dict]] = [None] * len(utts)
    for idx in plan_batches([u.length for u in utts], max_batch, max_pad_ratio):
        batch, kw = _bucket_inputs(model, utts, idx, dev, None, gvec)
        y_len = [int(specs[i].shape[1]) for i in idx]
        y = torch.zeros(len(idx), S, max(y_len), dtype=torch.float32, device=dev)
        for r, i in enumerate(idx):
            y[r, :, :y_len[r]] = specs[i].to(dev, torch.float32)
        out = model.score(batch["x"], [utts[i].length for i in idx], batch["sid"], batch["tone"], batch["language"], batch["bert"],
                          batch["ja_bert"], batch["en_bert"], y, y_len, g=kw.get("g"), seeds=kw.get("seeds"),
                          durations=kw["w_ceil"] if use_durations else None)
        host = {k: out[k].cpu().numpy() for k in ("nll", "nll_sym", "kl", "kl_frame", "durations", "l_length_dp", "l_length_sdp_mse")}
        path = None if out["score"] is None else out["score"].cpu().numpy()
        for r, i in enumerate(idx):
            n = utts[i].length
            res = dict(nll=host["nll"][r], nll_sym=host["nll_sym"][r, :n].copy(), kl=host["kl"][r], kl_frame=host["kl_frame"][r, :y_len[r]].copy(),
                       durations=host["durations"][r, :n].astype(np.int64), l_length_dp=host["l_length_dp"][r],
                       l_length_sdp_mse=host["l_length_sdp_mse"][r])
            if path is not None:
                res["score"] = path[r]
            results[i] = res
    return results
