"""Length-bucketed batches: a bounded ladder of step shapes for variable-length data.  No reference counterpart: the
reference batches in manifest order and pads every batch to its own longest utterance (data_loader.py:149-163).

Everything fast in this package is keyed on the exact step shape (N, T): kernel plans are measured once per shape
(engine._tune_once) and a step is replayed from a recorded launch list only once its shape has come back (replay.py).  Padding
every batch to its own longest utterance gives a stream of shapes that never repeats.  Here every batch is padded to one of a
few *rungs* instead:

    nominal_frames(dataset)      feature frames of every manifest row, from the duration column or the file header
    choose_ladder(frames, K)     the K rungs (multiples of ``align``) with the least total padding: the exact optimum
    BucketBatchSampler(...)      batches cut from one rung at a time, sharded by rank, shuffled by a private generator
    rung_for(ladder, t, align)   the width a batch whose longest utterance has ``t`` frames is padded to

Host code only (numpy and torch's CPU generator): this module imports and runs without a GPU."""
from __future__ import annotations

import math
import wave
from typing import List, Sequence, Tuple

import numpy as np
import torch

from .resample import output_length, resample_ratio


def _header(path) -> Tuple[int, int]:
    """(sample frames, sample rate) of an audio file from its header: soundfile when it is installed, otherwise the standard
    library's WAV reader (the fallback order of data_loader._sample_rate)"""
    try:
        import soundfile as sf
        info = sf.info(path)
        return int(info.frames), int(info.samplerate)
    except ImportError:
        pass
    try:
        with wave.open(path, 'rb') as w:                  # the header only
            return int(w.getnframes()), int(w.getframerate())
    except wave.Error:
        from .data_loader import _read_wav                # IEEE-float WAV: no header-only reader without soundfile
        data, sr = _read_wav(path)
        return int(data.shape[0]), int(sr)


def nominal_frames(dataset) -> np.ndarray:
    """int64 [len(dataset)]: the feature frames of every manifest row of a SpectrogramDataset without decoding audio.  The
    sample count is ``int(duration * rate)`` where the manifest has a duration above 0 (what load_audio reads), otherwise the
    file's length minus ``int(offset * rate)``; with ``dataset.resample`` it is converted to the model's rate exactly as the
    resampler does (ceil(n * model rate / file rate)).  Frames = 1 + samples // hop (SpectrogramExtractor.n_frames).  Speed
    perturbation is not in these numbers: choose_ladder's ``headroom`` covers it.  Cached on the dataset."""
    cached = getattr(dataset, '_nominal_frames', None)
    if cached is not None and len(cached) == len(dataset.rows):
        return cached
    model_rate = int(dataset.sample_rate)
    hop = int(model_rate * dataset.window_stride)
    resample = bool(getattr(dataset, 'resample', False))
    out = np.zeros(len(dataset.rows), dtype=np.int64)
    for i, r in enumerate(dataset.rows):
        duration, offset = float(r.get('duration', -1)), float(r.get('offset', 0))
        total = rate = None
        if resample or duration <= 0:
            total, rate = _header(r['audio_filepath'])
        if not resample:
            rate = model_rate
        if duration > 0:
            n = int(duration * rate)
        else:
            n = max(total - (int(offset * rate) if offset > 0 else 0), 0)
        if resample and rate != model_rate:
            n = output_length(n, resample_ratio(rate, model_rate))
        out[i] = 1 + n // hop
    dataset._nominal_frames = out
    return out


def _round_up(t, align: int):
    return -(-t // align) * align


def ladder_cost(frames, ladder) -> int:
    """sum over ``frames`` of the smallest rung at or above each (the padded frames of a perfect packing, valid ones included)"""
    frames = np.asarray(frames, dtype=np.int64)
    rungs = np.asarray(ladder, dtype=np.int64)
    idx = np.searchsorted(rungs, frames, side='left')
    if len(frames) and idx.max() >= len(rungs):
        raise ValueError(f'a length of {int(frames.max())} frames is above the top rung {int(rungs[-1])}')
    return int(rungs[idx].sum())


def choose_ladder(frames, rungs: int, align: int = 16, headroom: float = 1.0) -> List[int]:
    """At most ``rungs`` ascending rungs, each a multiple of ``align``, the top one at least ceil(max(frames) * headroom), that
    minimise ladder_cost(frames, .).  Exact: an optimal rung sits on the aligned length of some utterance (lowering a rung to
    the longest aligned length below it changes no assignment and no cost upwards), so the search is a dynamic program over the
    distinct aligned lengths v_1 < ... < v_m with counts prefix C:

        best[k][j] = min_{i < j} best[k-1][i] + v_j * (C_j - C_i)        (k rungs, the k-th at v_j, all lengths <= v_j covered)

    Deterministic: among equal costs the fewer rungs win, then the lower split point.  ``headroom`` = 1 / min(speed factors)
    with speed perturbation: only the top rung is raised (a slowed-down batch may land one rung higher; none leaves the ladder)."""
    frames = np.asarray(frames, dtype=np.int64).reshape(-1)
    rungs, align = int(rungs), int(align)
    if rungs < 1 or align < 1:
        raise ValueError(f'rungs and align must be at least 1, got {rungs} and {align}')
    if not len(frames):
        raise ValueError('no lengths to choose a ladder from')
    if frames.min() < 1 or headroom < 1.0:
        raise ValueError('lengths must be positive and headroom at least 1')
    v, counts = np.unique(_round_up(frames, align), return_counts=True)
    top = _round_up(max(int(math.ceil(int(frames.max()) * float(headroom))), int(v[-1])), align)
    if top > v[-1]:                                       # the forced top rung: a candidate that no nominal length needs
        v, counts = np.append(v, top), np.append(counts, 0)
    m = len(v)
    C = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)           # C[j]: rows with aligned length <= v[j-1]
    INF = np.iinfo(np.int64).max // 4
    best = np.full((rungs + 1, m + 1), INF, dtype=np.int64)                 # column j: the k-th rung is v[j-1]; column 0: none yet
    back = np.zeros((rungs + 1, m + 1), dtype=np.int64)
    best[0, 0] = 0
    for k in range(1, rungs + 1):
        for j in range(k, m + 1):
            cand = best[k - 1, :j] + v[j - 1] * (C[j] - C[:j])
            i = int(np.argmin(cand))                      # (first minimum: the lower split point)
            best[k, j], back[k, j] = min(cand[i], INF), i
    k = int(np.argmin(best[1:, m])) + 1                   # (first minimum: the fewer rungs)
    ladder, j = [], m
    while k > 0:
        ladder.append(int(v[j - 1]))
        j, k = int(back[k, j]), k - 1
    return ladder[::-1]


def rung_for(ladder: Sequence[int], t: int, align: int = 16) -> Tuple[int, bool]:
    """(width, on the ladder): the smallest rung at or above ``t``; above the top rung, the next multiple of ``align``"""
    for r in ladder:
        if r >= t:
            return int(r), True
    return int(_round_up(int(t), int(align))), False


class BucketBatchSampler(torch.utils.data.Sampler):
    """Batch sampler over rows of known length (``frames``: nominal_frames) for a ladder of rungs.  Rows are grouped by their
    rung; global batches of ``batch_size * num_replicas`` rows are cut from one rung at a time, lowest first, and the leftover
    rows of a rung (fewer than a global batch) are carried into the next rung up, so that at most one batch is short: the final
    remainder, which is dropped with ``drop_last`` and otherwise padded to a multiple of ``num_replicas`` by repeating rows of
    its highest rung (every rank takes the same number of steps; a rank that ran out of batches early would leave the others
    waiting in a collective).  Inside a global batch the rows are sorted by length and rank r takes rows r::num_replicas: with
    ``num_replicas`` rows of the batch's highest rung in every batch -- carried rows are placed accordingly, which needs
    ``batch_size`` >= 2 and no rung with fewer rows than ranks -- every rank runs the same rung at the same step, with
    near-equal valid frames.  ``shuffle``: the order inside each rung and the order of the
    batches come from a private torch.Generator seeded ``seed + epoch`` (set_epoch), the same on every rank; neither Python's
    nor torch's global generator is touched.  Rows above the top rung ride in the top rung's batches (the loader pads such a
    batch past the ladder and counts it).  ``padded_frames`` / ``valid_frames``: the pad and the valid frames of the epoch last
    planned, over all ranks, each batch at the rung of its longest row."""

    def __init__(self, frames, batch_size: int, ladder: Sequence[int], shuffle: bool = True, seed: int = 0,
                 drop_last: bool = False, num_replicas: int = 1, rank: int = 0):
        self.frames = np.asarray(frames, dtype=np.int64).reshape(-1)
        self.batch_size, self.num_replicas, self.rank = int(batch_size), int(num_replicas), int(rank)
        self.ladder = [int(r) for r in ladder]
        if self.batch_size < 1 or self.num_replicas < 1 or not 0 <= self.rank < self.num_replicas:
            raise ValueError(f'batch_size {batch_size}, num_replicas {num_replicas}, rank {rank}')
        if not self.ladder or any(b <= a for a, b in zip(self.ladder, self.ladder[1:])):
            raise ValueError(f'a ladder is a non-empty ascending list of rungs, got {ladder!r}')
        self.shuffle, self.seed, self.drop_last = bool(shuffle), int(seed), bool(drop_last)
        self.epoch = 0
        self._plan()

    def set_epoch(self, epoch: int):
        self.epoch = int(epoch)
        self._plan()

    def _plan(self):
        R, G = self.num_replicas, self.batch_size * self.num_replicas
        gen = torch.Generator().manual_seed(self.seed + self.epoch)
        top = len(self.ladder) - 1
        of_row = np.minimum(np.searchsorted(np.asarray(self.ladder), self.frames, side='left'), top)
        batches, carried = [], np.zeros(0, dtype=np.int64)
        for k in range(top + 1):
            rows = np.flatnonzero(of_row == k)
            if self.shuffle and len(rows) > 1:
                rows = rows[torch.randperm(len(rows), generator=gen).numpy()]
            # the batch that takes the carried rows keeps room for R rows of this rung (one per rank); carried rows beyond that
            # wait for the next batch
            keep = min(len(carried), G - R)
            rows = np.concatenate([carried[:keep], rows[:R], carried[keep:], rows[R:]])
            full = len(rows) // G * G
            batches += [rows[i:i + G] for i in range(0, full, G)]
            carried = rows[full:]
        if self.shuffle and len(batches) > 1:
            batches = [batches[i] for i in torch.randperm(len(batches), generator=gen).tolist()]
        if len(carried) and not self.drop_last:           # the one short batch runs last
            highest = carried[of_row[carried] == of_row[carried].max()]
            extra = max(R - len(highest), 0)              # one row of the highest rung per rank, then a multiple of R rows
            extra += -(len(carried) + extra) % R
            batches.append(np.concatenate([carried, np.resize(highest, extra)]))         # (np.resize repeats the rows in order)
        self.padded_frames = self.valid_frames = 0
        self._batches = []
        for b in batches:
            b = b[np.lexsort((b, self.frames[b]))]        # by length, ties by row index
            valid = int(self.frames[b].sum())
            self.valid_frames += valid
            self.padded_frames += rung_for(self.ladder, int(self.frames[b[-1]]), 1)[0] * len(b) - valid
            self._batches.append(b)

    def global_batches(self) -> List[List[int]]:
        """the epoch's batches before sharding: row indices sorted by length"""
        return [b.tolist() for b in self._batches]

    def __iter__(self):
        for b in self._batches:
            yield b[self.rank::self.num_replicas].tolist()

    def __len__(self):
        return len(self._batches)
