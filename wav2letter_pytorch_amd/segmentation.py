"""Long-form transcription: voice activity detection on the GPU (csrc/vad.hip), segmentation of a recording at its pauses,
and ``transcribe_long`` -- the pieces go through the model as the utterances it was trained on, text and word times come back
on the recording's clock.  No reference counterpart: the reference transcribes utterances only.

The rule (DESIGN.md "Long-form transcription" has it in full; tests/vad_refs.py restates it in numpy): frame power in fp64,
``floor`` = the q-quantile and ``peak`` = the largest frame power, ``thr_on = max(abs_min, min(floor * r_on, sqrt(floor * peak)))``,
``thr_off = thr_on * r_hyst``, hysteresis between the two, gaps shorter than ``min_silence`` closed, runs shorter than
``min_speech`` dropped, every run widened by ``pad``, and a run longer than ``max_seconds`` cut at its quietest frame.  The
defaults are conventions; they are not tuned on speech (there is no speech corpus where this was written).

``find_keywords`` runs the same pieces through the keyword search (keyword_search.py) instead of, or as well as, a decoder.

This module imports without a GPU: only ``vad_segments``, ``transcribe_long`` and ``find_keywords`` touch the device."""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import List, Optional, Sequence

import numpy as np

INITIAL_CAP = 256            # segments per recording the first launch has room for (grown once when a recording has more)
MAX_FRAMES = 1 << 24         # w2l_vad_segments takes fewer frames than this per recording
HEADER_BYTES = 32            # W2L_VAD_HEADER_BYTES


@dataclass
class VadConfig:
    """The numbers of the rule in seconds and dB, and the analysis frames they are counted in.  ``on_dbfs`` (with ``off_dbfs``,
    default ``on_dbfs - hyst_db``): absolute thresholds instead of the adaptive ones, as frame power relative to a full-scale
    square wave, 10^(dBFS / 10).  ``sample_rate`` / ``window_size`` / ``window_stride``: the model's ``audio_conf`` values."""
    q: float = 0.05
    on_db: float = 10.0
    hyst_db: float = 3.0
    abs_min: float = 1e-10
    min_silence: float = 0.30
    min_speech: float = 0.10
    pad: float = 0.20
    on_dbfs: Optional[float] = None
    off_dbfs: Optional[float] = None
    sample_rate: int = 16000
    window_size: float = 0.02
    window_stride: float = 0.01

    def __post_init__(self):
        self.sample_rate = int(self.sample_rate)
        self.win = int(self.sample_rate * self.window_size)
        self.hop = int(self.sample_rate * self.window_stride)
        if self.hop < 1 or self.hop > self.win:
            raise ValueError(f'window_stride must give 1 <= hop <= win samples (hop={self.hop}, win={self.win})')
        self.n_fft = 2 ** math.ceil(math.log2(self.win))
        for name in ('q', 'on_db', 'hyst_db', 'abs_min', 'min_silence', 'min_speech', 'pad'):
            setattr(self, name, float(getattr(self, name)))
            if not math.isfinite(getattr(self, name)):
                raise ValueError(f'{name}={getattr(self, name)!r} is not finite')
        if not 0.0 <= self.q <= 1.0:
            raise ValueError(f'q={self.q} outside [0, 1]')
        if self.hyst_db < 0:
            raise ValueError(f'hyst_db={self.hyst_db} is negative: thr_off would lie above thr_on')
        if self.abs_min < 0 or self.min_silence < 0 or self.pad < 0:
            raise ValueError('abs_min, min_silence and pad must not be negative')
        if self.off_dbfs is not None and self.on_dbfs is None:
            raise ValueError('off_dbfs is given without on_dbfs')
        if self.on_dbfs is not None:
            self.on_dbfs = float(self.on_dbfs)
            self.off_dbfs = self.on_dbfs - self.hyst_db if self.off_dbfs is None else float(self.off_dbfs)
            if not (math.isfinite(self.on_dbfs) and math.isfinite(self.off_dbfs)) or self.off_dbfs > self.on_dbfs:
                raise ValueError(f'absolute thresholds must be finite with off_dbfs <= on_dbfs ({self.on_dbfs}, {self.off_dbfs})')
        # the shortest segment the rule can emit is a run of min_speech frames whose last frame is partial; the front end
        # pads it by reflection, which needs more than n_fft / 2 samples
        if self.shortest_samples(self.frames(self.min_speech)) <= self.n_fft // 2:
            raise ValueError(f'min_speech={self.min_speech} s allows segments of {self.shortest_samples(self.frames(self.min_speech))} '
                             f'samples, not above the front end\'s reflect padding ({self.n_fft // 2} samples)')

    @classmethod
    def for_model(cls, audio_conf, **kw):
        return cls(sample_rate=audio_conf['sample_rate'], window_size=audio_conf['window_size'],
                   window_stride=audio_conf['window_stride'], **kw)

    def frames(self, seconds: float) -> int:
        """a duration in analysis frames, rounded to the nearest"""
        return int(round(float(seconds) * self.sample_rate / self.hop))

    def shortest_samples(self, frames: int) -> int:
        """samples of the shortest recording stretch that ``frames`` frames can cover (the last one partial)"""
        return (frames - 1) * self.hop + 1 if frames >= 1 else 0

    def numbers(self, max_seconds: float = 20.0) -> dict:
        """the fields of w2l_vad_params_t: frame counts, and the ratios both device and reference multiply by"""
        max_frames = int(math.floor(float(max_seconds) * self.sample_rate / self.hop))
        if max_frames < 2:
            raise ValueError(f'max_seconds={max_seconds} is {max_frames} frames: at least 2 are needed')
        if self.shortest_samples(max_frames // 2) <= self.n_fft // 2:
            raise ValueError(f'max_seconds={max_seconds} allows forced pieces of {self.shortest_samples(max_frames // 2)} samples, '
                             f'not above the front end\'s reflect padding ({self.n_fft // 2} samples)')
        absolute = self.on_dbfs is not None
        return dict(q=self.q, r_on=10.0 ** (self.on_db / 10.0), r_hyst=10.0 ** (-self.hyst_db / 10.0), abs_min=self.abs_min,
                    thr_on=10.0 ** (self.on_dbfs / 10.0) if absolute else 0.0,
                    thr_off=10.0 ** (self.off_dbfs / 10.0) if absolute else 0.0, absolute=int(absolute),
                    min_silence=self.frames(self.min_silence), min_speech=self.frames(self.min_speech), pad=self.frames(self.pad),
                    max_frames=max_frames)


def vad_params(numbers: dict):
    """w2l_vad_params_t from ``VadConfig.numbers()`` (or a dict with its keys)"""
    from ._lib import VadParams
    p = VadParams()
    for k, v in numbers.items():
        setattr(p, k, v)
    return p


def parse_records(buf: np.ndarray, n: int, cap: int) -> List[dict]:
    """the output buffer of w2l_vad_segments (uint8, host) -> one dict per recording"""
    stride = HEADER_BYTES + 8 * cap
    out = []
    for i in range(n):
        rec = buf[i * stride: (i + 1) * stride]
        count, status = (int(v) for v in rec[:8].view(np.int32))
        thr_on, thr_off = (float(v) for v in rec[8:24].view(np.float64))
        floor, peak = rec[24:32].view(np.float32)
        segs = rec[HEADER_BYTES:].view(np.int32).reshape(cap, 2)[:min(count, cap)].astype(np.int64)
        out.append(dict(count=count, status=status, thr_on=thr_on, thr_off=thr_off, floor=floor, peak=peak, frames=segs))
    return out


def segments_from_power(power, nframes_dev, numbers: dict, cap: int = INITIAL_CAP, grow: bool = True) -> List[dict]:
    """the decision launch on device powers [N, Fmax] (fp32, contiguous) and frame counts [N] (int32, device): one launch, one
    copy to the host; with ``grow`` ``cap`` is raised and the launch repeated once when a recording has more segments (status
    bit 0)"""
    import ctypes as C
    import torch
    from ._lib import check, lib, ptr, stream_ptr
    n, fmax = power.shape
    if fmax >= MAX_FRAMES:
        raise ValueError(f'a recording of {fmax} frames: the segmentation takes fewer than 2^24 frames per recording')
    params = vad_params(numbers)
    ws_bytes = int(lib.w2l_vad_workspace_bytes(n, fmax))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=power.device)
    for _ in range(2):
        out = torch.empty(n * (HEADER_BYTES + 8 * cap), dtype=torch.uint8, device=power.device)
        check(lib.w2l_vad_segments(ptr(power), fmax, ptr(nframes_dev), n, C.byref(params), cap, ptr(ws), ws_bytes, ptr(out),
                                   stream_ptr()), 'w2l_vad_segments')
        recs = parse_records(out.cpu().numpy(), n, cap)
        most = max(r['count'] for r in recs)
        if most <= cap or not grow:
            break
        cap = most
    return recs


def frame_power(x, lens_dev, fmax: int, win: int, hop: int):
    """the power launch: device rows x [N, L] (fp32, contiguous) and lengths [N] (int32, device) -> powers [N, fmax]"""
    import torch
    from ._lib import check, lib, ptr, stream_ptr
    power = torch.empty(x.shape[0], fmax, dtype=torch.float32, device=x.device)
    check(lib.w2l_vad_power(ptr(x), x.shape[1], ptr(lens_dev), x.shape[0], win, hop, ptr(power), fmax, stream_ptr()), 'w2l_vad_power')
    return power


def vad_segments(waves, cfg: Optional[VadConfig] = None, max_seconds: float = 20.0, return_stats: bool = False):
    """waves: N recordings at the model's rate, each a 1-D device tensor or array (one recording may be passed bare) -> per
    recording an int64 [S, 2] array of half-open sample ranges, ascending; a recording of silence gives [0, 2].  Two launches
    (frame power, decisions) and one copy to the host.  ``return_stats``: (segments, stats) with per recording a dict of
    count, status, thr_on, thr_off, floor, peak and the segments in frames."""
    import torch
    cfg = cfg or VadConfig()
    numbers = cfg.numbers(max_seconds)
    if torch.is_tensor(waves) and waves.dim() == 1 or isinstance(waves, np.ndarray) and waves.ndim == 1:
        waves = [waves]
    waves = list(waves)
    dev = next((w.device for w in waves if torch.is_tensor(w) and w.is_cuda), None)
    if dev is None:
        if not torch.cuda.is_available():
            raise RuntimeError('vad_segments runs on MI355X only (HIP kernels, no CPU path)')
        dev = torch.device('cuda', torch.cuda.current_device())
    rows = [w.reshape(-1) if torch.is_tensor(w) else torch.from_numpy(np.ascontiguousarray(np.asarray(w, dtype=np.float32).reshape(-1)))
            for w in waves]
    lens = np.array([int(r.shape[0]) for r in rows], dtype=np.int64)
    nfr = -(-lens // cfg.hop)
    fmax = max(1, int(nfr.max()))
    if fmax >= MAX_FRAMES:
        raise ValueError(f'a recording of {fmax} frames ({int(lens.max())} samples): the segmentation takes fewer than 2^24 frames '
                         'per recording')
    if len(rows) == 1 and rows[0].is_cuda and rows[0].dtype == torch.float32 and rows[0].is_contiguous() and lens[0] > 0:
        x = rows[0].view(1, -1)                          # the recording as it lies on the device: no copy
    else:
        x = torch.zeros(len(rows), max(1, int(lens.max())), dtype=torch.float32, device=dev)
        for i, r in enumerate(rows):
            x[i, :r.shape[0]] = r.to(device=dev, dtype=torch.float32)
    with torch.cuda.device(dev):
        ints = torch.from_numpy(np.concatenate([lens, nfr]).astype(np.int32)).to(dev)
        power = frame_power(x, ints[:len(rows)], fmax, cfg.win, cfg.hop)
        recs = segments_from_power(power, ints[len(rows):], numbers)
    segs = []
    for r, n in zip(recs, lens):
        fr = r['frames']
        segs.append(np.stack([fr[:, 0] * cfg.hop, np.minimum(int(n), fr[:, 1] * cfg.hop)], 1).astype(np.int64).reshape(-1, 2))
    return (segs, recs) if return_stats else segs


# ---------------------------------------------------------------------------------------------------------------- stitching
def stitch(pieces: Sequence[dict], sample_rate: int, word_times: bool = False) -> dict:
    """pieces: per segment {'start': first sample, 'end': one past the last, 'text': ..., 'words': [(word, s, e), ...] on the
    SEGMENT's clock} in any order -> the result of one recording: ``text`` = the non-empty segment texts joined by one space in
    time order, ``segments`` with start / end in seconds on the recording's clock, and -- with ``word_times`` -- ``words`` as
    {'word', 'start', 'end'} with the segment's start added."""
    segs = []
    for p in sorted(pieces, key=lambda p: p['start']):
        t0 = p['start'] / float(sample_rate)
        seg = {'start': t0, 'end': p['end'] / float(sample_rate), 'text': p['text']}
        if word_times:
            seg['words'] = [{'word': w, 'start': t0 + float(s), 'end': t0 + float(e)} for w, s, e in (p.get('words') or [])]
        segs.append(seg)
    return {'text': ' '.join(s['text'] for s in segs if s['text'].strip()), 'segments': segs}


def batches_by_length(lengths: Sequence[int], batch_size: int) -> List[List[int]]:
    """segment indices grouped into batches of neighbours in length (longest first), so a batch pads little"""
    order = sorted(range(len(lengths)), key=lambda i: (-int(lengths[i]), i))
    bs = max(1, int(batch_size))
    return [order[i: i + bs] for i in range(0, len(order), bs)]


def _device_wave(model, ext, item, model_rate, dev):
    """one input of transcribe_long -> its waveform at the model's rate, fp32 [L] on the device (uploaded once; other rates go
    through the device resampler)"""
    import torch
    from .data.data_loader import read_audio
    from .data.resample import plan_rows, resample_device
    if isinstance(item, str):
        audio, rate = read_audio(item)
    elif isinstance(item, tuple) and len(item) == 2:
        audio, rate = item[0], int(item[1])
    else:
        audio, rate = item, model_rate
    if torch.is_tensor(audio):
        wave = audio.detach().reshape(-1).to(device=dev, dtype=torch.float32)
    else:
        wave = torch.from_numpy(np.ascontiguousarray(np.asarray(audio, dtype=np.float32).reshape(-1))).to(dev)
    if rate == model_rate or wave.numel() == 0:
        return wave.contiguous()
    n_in = int(wave.numel())
    n_out = -(-n_in * model_rate // rate)
    if max(n_in, n_out) >= 2 ** 31:
        raise ValueError(f'a recording of {n_in} samples at {rate} Hz ({n_out} at {model_rate} Hz): the device resampler takes '
                         'fewer than 2^31 samples per row; split the file first')
    rows = plan_rows([n_in], [rate], model_rate, None, ext._banks)
    return resample_device(wave.view(1, -1).contiguous(), rows, ext._banks)[0, :int(rows[0, 1])].contiguous()


def for_each_piece(model, items, max_seconds: float, batch_size: int, vad: Optional[VadConfig], handle, finish) -> list:
    """the loop ``transcribe_long`` and ``find_keywords`` share: every input uploaded once, cut at its pauses on the device, the
    pieces batched with neighbours in length through the front end and ``model.infer``.  ``handle(batch, segs, out, out_lens)``
    turns the posteriors of one batch (``batch``: the piece indices into ``segs``, int64 [S, 2] sample ranges) into a list of
    per-piece records; ``finish(records, sample_rate)`` makes one input's result of them -> the results, in input order."""
    import torch
    from .data.data_loader import SpectrogramExtractor
    items = [items] if isinstance(items, str) or torch.is_tensor(items) or isinstance(items, np.ndarray) and items.ndim == 1 \
        else list(items)
    dev = next(model.parameters()).device
    ext = model.__dict__.get('_transcribe_extractor')
    if ext is None or ext.fb.device != dev:
        ext = model.__dict__['_transcribe_extractor'] = SpectrogramExtractor(model.audio_conf, model._cfg.input_size, device=dev)
    model_rate = int(model.audio_conf['sample_rate'])
    vad = vad or VadConfig.for_model(model.audio_conf)
    if (vad.sample_rate, vad.win, vad.hop) != (model_rate, ext.win_length, ext.hop_length):
        raise ValueError(f'the VadConfig is for {vad.sample_rate} Hz with frames of {vad.win} / {vad.hop} samples; the model has '
                         f'{model_rate} Hz and {ext.win_length} / {ext.hop_length}')
    vad.numbers(max_seconds)                             # (argument errors before any file is read)
    was_training = model.training
    model.eval()
    results = []
    try:
        with torch.no_grad(), torch.cuda.device(dev):
            for item in items:
                wave = _device_wave(model, ext, item, model_rate, dev)
                segs = vad_segments([wave], vad, max_seconds)[0] if wave.numel() else np.zeros((0, 2), dtype=np.int64)
                lengths = (segs[:, 1] - segs[:, 0]).tolist()
                pieces = []
                for batch in batches_by_length(lengths, batch_size):
                    lens = np.array([lengths[i] for i in batch], dtype=np.int32)
                    rows = torch.zeros(len(batch), int(lens.max()), dtype=torch.float32, device=dev)
                    for j, i in enumerate(batch):
                        rows[j, :lens[j]] = wave[int(segs[i, 0]): int(segs[i, 1])]
                    x, x_lens = ext.extract_rows(rows, lens)
                    out, out_lens = model.infer(x, x_lens)
                    pieces += handle(batch, segs, out, out_lens)
                results.append(finish(pieces, model_rate))
    finally:
        if was_training:
            model.train()
    return results


def transcribe_long(model, items, max_seconds: float = 20.0, batch_size: int = 8, decoder=None, word_times: bool = False,
                    vad: Optional[VadConfig] = None) -> List[dict]:
    """the body of ``ConvCTCASR.transcribe_long`` (its docstring has the interface)"""
    from .evaluate import decode_batch
    decoder = decoder or model.ctc_decoder

    def handle(batch, segs, out, out_lens):
        hyps, words = decode_batch(model, decoder, out, out_lens, word_times)
        return [{'start': int(segs[i, 0]), 'end': int(segs[i, 1]), 'text': hyp, 'words': w} for i, hyp, w in zip(batch, hyps, words)]

    return for_each_piece(model, items, max_seconds, batch_size, vad, handle,
                          lambda pieces, rate: stitch(pieces, rate, word_times))


def find_keywords(model, items, phrases, threshold: float = -1.0, max_hits: int = 8, max_seconds: float = 20.0,
                  batch_size: int = 8, vad: Optional[VadConfig] = None, also_transcribe: bool = False, decoder=None):
    """the body of ``ConvCTCASR.find_keywords`` (its docstring has the interface)"""
    from .evaluate import decode_batch, frame_seconds
    from .keyword_search import KeywordTable, ctc_keyword_search
    if getattr(getattr(model, 'criterion', None), 'is_asg', False):
        raise NotImplementedError('find_keywords on a model with criterion asg: the keyword search is the CTC recurrence (a blank '
                                  'between repeated letters, no transitions); the ASG recurrence is not built')
    blank = int(model.ctc_decoder.blank_index)
    table = phrases if isinstance(phrases, KeywordTable) else \
        KeywordTable([phrases] if isinstance(phrases, str) else list(phrases), labels=list(model.labels), blank=blank)
    names = [text if text is not None else list(kw) for text, kw in zip(table.texts, table.keywords)]
    ratio = frame_seconds(model)
    log_probs = bool(getattr(model, 'infer_log_probs', True))
    decoder = decoder or model.ctc_decoder

    def handle(batch, segs, out, out_lens):
        found = ctc_keyword_search(out, table, input_lengths=out_lens, blank=blank, log_probs=log_probs, threshold=threshold,
                                   max_hits=max_hits)
        recs = [{'start': int(segs[i, 0]), 'end': int(segs[i, 1]), 'hits': hits} for i, hits in zip(batch, found)]
        if also_transcribe:
            for rec, hyp in zip(recs, decode_batch(model, decoder, out, out_lens, False)[0]):
                rec.update(text=hyp, words=None)
        return recs

    def finish(pieces, rate):
        hits = []
        for p in pieces:
            t0 = p['start'] / float(rate)
            hits += [{'keyword': names[k], 'start': t0 + float(s * ratio), 'end': t0 + float(e * ratio), 'score': sc}
                     for k, s, e, sc in p['hits']]
        hits.sort(key=lambda h: (h['start'], h['end']))
        return (hits, stitch(pieces, rate)) if also_transcribe else hits

    return for_each_piece(model, items, max_seconds, batch_size, vad, handle, finish)


# ------------------------------------------------------------------------------- a whole transcript against a whole recording
def transcript_lines(text):
    """``text`` (a string: one line; or a list of strings: lines or sentences) -> (joined, spans): runs of whitespace collapse
    to one space, lines are joined by one space, ``spans[i]`` is the half-open character range of line i in ``joined``.  A line
    without a character is a ValueError (it would have no place on the clock)."""
    lines = [text] if isinstance(text, str) else list(text)
    if not lines:
        raise ValueError('align_transcript: no text')
    spans, parts, at = [], [], 0
    for i, line in enumerate(lines):
        if not isinstance(line, str):
            raise ValueError(f'align_transcript: line {i} is {type(line).__name__}, not a string')
        line = ' '.join(line.split())
        if not line:
            raise ValueError(f'align_transcript: line {i} holds no character')
        spans.append((at, at + len(line)))
        parts.append(line)
        at += len(line) + 1
    return ' '.join(parts), spans


def word_spans(joined: str):
    """[(word, first character, one past its last)] of a string whose words are separated by single spaces"""
    out, at = [], 0
    for w in joined.split(' '):
        if w:
            out.append((w, at, at + len(w)))
        at += len(w) + 1
    return out


def frame_times(frames, table, sample_rate: int, ratio: float):
    """frames of the concatenated posteriors -> seconds on the recording's clock.  ``table``: per piece in time order (first
    sample in the recording, first frame in the concatenation); a frame belongs to the last piece that starts at or before it and
    lies at that piece's start plus its frame offset times ``ratio`` (seconds per frame), transcribe_long's word-time convention.
    Silence the VAD dropped has no frames, so time jumps between pieces."""
    table = np.asarray(table, dtype=np.int64).reshape(-1, 2)
    frames = np.asarray(frames, dtype=np.int64)
    if table.shape[0] < 1 or (np.diff(table[:, 1]) <= 0).any() or table[0, 1] != 0:
        raise ValueError('frame_times: the piece table needs first frames ascending from 0')
    if frames.size and (frames.min() < 0):
        raise ValueError('frame_times: a negative frame')
    piece = np.searchsorted(table[:, 1], frames, side='right') - 1
    return table[piece, 0] / float(sample_rate) + (frames - table[piece, 1]) * float(ratio)


def alignment_records(joined: str, line_spans, starts, ends, frame_logp, table, sample_rate: int, ratio: float) -> dict:
    """the result of align_transcript from the alignment of ``joined`` (``starts`` / ``ends``: first / last frame of each of its
    characters; ``frame_logp`` [T]: the log-posterior of the path's label at each frame) -> {'score', 'words', 'segments'}.  A
    word or line starts at its first character's first frame and ends at its last character's last frame, each on the clock of
    the piece the frame came from (a word cut by a piece boundary takes its start from one piece and its end from the next);
    its score is the mean of frame_logp over those frames."""
    starts, ends = np.asarray(starts, dtype=np.int64), np.asarray(ends, dtype=np.int64)
    cum = np.concatenate(([0.0], np.cumsum(np.asarray(frame_logp, dtype=np.float64))))

    def record(key, what, c0, c1):
        f0, f1 = int(starts[c0]), int(ends[c1 - 1])
        t0, t1 = frame_times([f0, f1], table, sample_rate, ratio)
        return {key: what, 'start': float(t0), 'end': float(t1), 'score': float((cum[f1 + 1] - cum[f0]) / (f1 + 1 - f0))}

    return {'score': float(cum[-1]),
            'words': [record('word', w, c0, c1) for w, c0, c1 in word_spans(joined)],
            'segments': [record('text', joined[c0:c1], c0, c1) for c0, c1 in line_spans]}


def align_transcript(model, item, text, max_seconds: float = 20.0, batch_size: int = 8, vad: Optional[VadConfig] = None) -> dict:
    """the body of ``ConvCTCASR.align_transcript`` (its docstring has the interface)"""
    import torch
    from .alignment import ctc_forced_align_long
    from .evaluate import frame_seconds
    if getattr(getattr(model, 'criterion', None), 'is_asg', False):
        raise NotImplementedError('align_transcript on a model with criterion asg: the long alignment is the CTC recurrence (a '
                                  'blank between repeated letters, no transitions); the ASG recurrence is not built')
    joined, spans = transcript_lines(text)
    labels = list(model.labels)
    for ch in joined:
        if ch not in labels:
            raise ValueError(f'align_transcript: character {ch!r} is not in the model\'s labels')
    blank = int(model.ctc_decoder.blank_index)
    log_probs = bool(getattr(model, 'infer_log_probs', True))
    ratio = frame_seconds(model)

    def handle(batch, segs, out, out_lens):
        lens = [out.shape[1]] * len(batch) if out_lens is None else [int(v) for v in torch.as_tensor(out_lens).cpu()]
        return [{'start': int(segs[i, 0]), 'end': int(segs[i, 1]), 'rows': out[j, :lens[j]]} for j, i in enumerate(batch)]

    def finish(pieces, rate):
        pieces = sorted((p for p in pieces if p['rows'].shape[0] > 0), key=lambda p: p['start'])
        frames = sum(p['rows'].shape[0] for p in pieces)
        if frames < len(joined):
            raise ValueError(f'align_transcript: {len(joined)} characters on {frames} frames of speech: no frame path spells the text')
        table, at = [], 0
        for p in pieces:
            table.append((p['start'], at))
            at += p['rows'].shape[0]
        x = torch.cat([p['rows'].float() for p in pieces], 0).contiguous()
        res = ctc_forced_align_long(x, joined, blank=blank, log_probs=log_probs, labels=labels)
        if not res.feasible[0]:
            raise ValueError(f'align_transcript: no frame path of {frames} frames spells the {len(joined)} characters of the text')
        path = torch.from_numpy(res.paths[0].astype(np.int64)).to(x.device)
        picked = x.gather(1, path.view(-1, 1)).view(-1)                # one gather: the path's label at every frame
        picked = (picked if log_probs else picked.log()).cpu().numpy()
        got = alignment_records(joined, spans, res.starts[0], res.ends[0], picked, table, rate, ratio)
        got['score'] = float(res.scores[0])
        return got

    return for_each_piece(model, [item], max_seconds, batch_size, vad, handle, finish)[0]
