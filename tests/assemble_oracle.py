"""numpy oracles of the document assembly (include/bv2.h bv2_assemble; test infrastructure, no test in here).

``reference_tail`` restates what reference webui.py does behind synthesis — ``generate_audio`` (gradio ``convert_to_16_bit_wav`` per
piece) and both branches of ``tts_split`` — operation for operation, dtype for dtype.  ``simple_document`` is the rule the device
implements: every piece under its own peak by ``bv2_pcm16``'s rule, zero pauses between.  ``assemble`` evaluates a timeline of segments
under the four level modes and two output formats the way include/bv2.h states them."""
import numpy as np

F32 = np.float32


def convert_to_16_bit_wav(data):
    """gradio.processing_utils.convert_to_16_bit_wav for the dtypes the reference hands it: floats are divided by their peak, multiplied
    by 32767 and cast (numpy's cast truncates toward zero); int16 passes through."""
    if data.dtype in (np.float64, np.float32, np.float16):
        data = data / np.abs(data).max()
        data = data * 32767
        return data.astype(np.int16)
    if data.dtype == np.int16:
        return data
    raise ValueError(data.dtype)


def reference_tail(paragraphs, interval_between_para, interval_between_sent, cut_by_sent):
    """``paragraphs``: a list of paragraphs, each a list of sentences, each a list of fp32 pieces (what ``infer`` returned).  The
    concatenated int16 audio of webui.py ``tts_split`` (:150-203), with ``process_text`` = ``generate_audio`` over the sentence's pieces."""
    audio_list = []
    for para in paragraphs:
        if not cut_by_sent:
            for sentence in para:
                audio_list += [convert_to_16_bit_wav(x) for x in sentence]
            audio_list.append(np.zeros(int(44100 * interval_between_para), dtype=np.int16))
        else:
            sent_list = []
            for sentence in para:
                sent_list += [convert_to_16_bit_wav(x) for x in sentence]
                sent_list.append(np.zeros(int(44100 * interval_between_sent)))            # float64, as the reference
            if interval_between_para - interval_between_sent > 0:
                sent_list.append(np.zeros(int(44100 * (interval_between_para - interval_between_sent))))
            audio_list.append(convert_to_16_bit_wav(np.concatenate(sent_list)))           # the second, fp64 normalisation
    return np.concatenate(audio_list)


def pcm16_rule(x, pk=None):
    """``bv2_pcm16``'s rule: ``(int16)(int)((x / pk) * 32767.f)`` in fp32, zeros where the peak is 0."""
    x = np.asarray(x, F32)
    if pk is None:
        pk = np.abs(x).max() if x.size else 0.0
    pk = F32(pk)
    if not pk > 0:
        return np.zeros(x.shape, np.int16)
    return ((x / pk).astype(F32) * F32(32767.0)).astype(F32).astype(np.int16)


def peak_f32(x, pk):
    x = np.asarray(x, F32)
    return (x / F32(pk)).astype(F32) if F32(pk) > 0 else np.zeros(x.shape, F32)


def gain_f32(x, g):
    return (np.asarray(x, F32) * F32(g)).astype(F32)


def gain_i16(x, g):
    """``bv2_loudness_apply``'s 16-bit rule: ``trunc(clamp((x * g) * 32767.f, -32768, 32767))``."""
    w = (gain_f32(x, g) * F32(32767.0)).astype(F32)
    return np.trunc(np.clip(w, F32(-32768.0), F32(32767.0))).astype(np.int16)


def pauses(rate, interval_between_para, interval_between_sent):
    """``(after a sentence, more after a paragraph's last, after a paragraph without cut_by_sent)`` in samples."""
    extra = interval_between_para - interval_between_sent
    return int(rate * interval_between_sent), int(rate * extra) if extra > 0 else 0, int(rate * interval_between_para)


def simple_document(paragraphs, interval_between_para, interval_between_sent, cut_by_sent, rate=44100, level=pcm16_rule):
    """Each piece through ``level`` (default: under its own peak), zero pauses between: the rule ``bv2_assemble`` implements.  The pieces
    may already be levelled (``level=lambda x: x``: joining what ``synthesize(as_pcm16=True)`` returned)."""
    sent, extra, para_only = pauses(rate, interval_between_para, interval_between_sent)
    out, dtype = [], None
    for para in paragraphs:
        for sentence in para:
            for x in sentence:
                out.append(level(x))
                dtype = out[-1].dtype
            if cut_by_sent:
                out.append(sent)
        out.append((extra if cut_by_sent else para_only))
    return np.concatenate([np.zeros(v, dtype) if isinstance(v, int) else v for v in out])


def assemble(segments, level, as_pcm16, gain=None):
    """``segments``: ``("piece", x fp32 array, group, doc)`` / ``("silence", n, doc)`` in timeline order.  Returns ``(one array per
    document, offsets per segment, totals per document)`` under ``level`` in ("none", "piece", "group", "gain")."""
    n_docs = max(s[-1] for s in segments) + 1
    peaks = {}
    for s in segments:
        if s[0] == "piece" and s[1].size:
            peaks[s[2]] = max(peaks.get(s[2], F32(0)), F32(np.abs(s[1]).max()))
    docs, offsets = [[] for _ in range(n_docs)], []
    at = [0] * n_docs
    for s in segments:
        d = s[-1]
        offsets.append(at[d])
        if s[0] == "silence":
            v = np.zeros(s[1], np.int16 if as_pcm16 else F32)
        else:
            x, g = np.asarray(s[1], F32), s[2]
            if level in ("piece", "group"):
                pk = (F32(np.abs(x).max()) if x.size else F32(0)) if level == "piece" else peaks.get(g, F32(0))
                v = pcm16_rule(x, pk) if as_pcm16 else peak_f32(x, pk)
            else:
                k = F32(1.0) if level == "none" or gain is None else F32(gain[g])
                v = gain_i16(x, k) if as_pcm16 else gain_f32(x, k)
        docs[d].append(v)
        at[d] += len(v)
    empty = np.zeros(0, np.int16 if as_pcm16 else F32)
    return [np.concatenate(v) if v else empty for v in docs], offsets, at
