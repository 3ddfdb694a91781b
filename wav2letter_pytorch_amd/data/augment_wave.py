"""Waveform augmentation of a batch on the GPU (csrc/augment.hip), between the resampler and the log-mel front end: room
reverberation, then additive noise at a drawn signal-to-noise ratio.  No reference counterpart: the reference augments
spectrograms only (data/augmentations.py).  Neither step changes a row's length.

Reverberation, for a row of ``n_in`` samples, a response ``h[0..K)`` and its direct-path index ``d``:

    out[m] = sum_{j < K} h[j] * x~[m + d - j],   0 <= m < n_in,   x~ = 0 outside [0, n_in)

``prepare_rir`` makes ``h`` from a recorded response on the host: mono, at the model's rate, ``d`` = the index of the largest
|h|, cut ``max_seconds`` after it, scaled in float64 to unit energy and rounded once to fp32.

Noise, for a row with a clip ``z[0..n_z)``, an offset ``o`` and ``snr_db``:

    Ps = mean_{m < n_in} x[m]^2,   Pz = mean_{m < n_in} z[(o + m) mod n_z]^2,   g = sqrt(Ps / (Pz * 10^(snr_db / 10)))
    out[m] = fmaf(g, z[(o + m) mod n_z], x[m])

A row without a response / clip, a silent utterance and a silent clip are copied bit for bit.  This module imports without a
GPU; only ``RirBank.device_tables``, ``reverb_device``, ``mix_noise_device`` and ``WaveformAugment.apply`` touch the device.
"""
from __future__ import annotations

import json
import random
from typing import List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

MAX_TAPS = 16384                 # W2L_REVERB_MAX_TAPS (include/w2l_hip.h): 1 s at 16 kHz
MAX_BANK_BYTES = 256 << 20       # a larger set of responses is refused (ValueError)


def parse_range(value) -> Tuple[float, float]:
    """the ``data.snr_db`` config key: '5,20', a list / tuple of two numbers, or one number (a fixed SNR) -> (lo, hi)"""
    if isinstance(value, str):
        value = [v for v in value.replace('[', '').replace(']', '').replace('(', '').replace(')', '').split(',') if v.strip()]
    elif isinstance(value, (int, float)):
        value = [value, value]
    value = [float(v) for v in value]
    if len(value) == 1:
        value = value * 2
    if len(value) != 2:
        raise ValueError(f'a range is two numbers lo,hi: {value!r}')
    lo, hi = value
    if not lo <= hi:
        raise ValueError(f'the range {lo},{hi} is reversed')
    return lo, hi


def prepare_rir(samples, file_rate: int, model_rate: int, max_seconds: float = 0.5):
    """(h float32 [K], d): the response ``reverb_device`` convolves with.  ``samples``: [n] or [n, channels] at ``file_rate``."""
    h = np.asarray(samples, dtype=np.float64)
    if h.ndim > 1:
        h = h.mean(axis=1)
    if int(file_rate) != int(model_rate):
        from .resample import resample_batch             # the GPU resampler: a response is audio like any other
        out, n_out = resample_batch([h.astype(np.float32)], [int(file_rate)], int(model_rate))
        h = out[0, :int(n_out[0])].cpu().numpy().astype(np.float64)
    if h.shape[0] == 0 or not np.any(h):
        raise ValueError('an impulse response needs at least one non-zero sample')
    p = int(np.argmax(np.abs(h)))
    h = h[:p + int(max_seconds * model_rate)]
    if h.shape[0] <= p:                                  # max_seconds rounds to no samples
        raise ValueError(f'rir_max_seconds={max_seconds} keeps no sample of the response')
    if h.shape[0] > MAX_TAPS:
        raise ValueError(f'the response keeps {h.shape[0]} taps (peak at {p}), above the supported {MAX_TAPS}: lower rir_max_seconds')
    h = h / np.sqrt(np.sum(h * h))
    return h.astype(np.float32), p


class RirBank:
    """The impulse responses of a manifest, modelled on resample.BankCache: prepared once on the host, concatenated, uploaded
    once, with the descriptor table {offset, K, d} that w2l_reverb reads."""

    def __init__(self, responses: Sequence[Tuple[np.ndarray, int]] = ()):
        self.desc = np.zeros((0, 3), dtype=np.int32)
        self._taps: List[np.ndarray] = []
        self._n_taps = 0
        self._taps_dev = None
        self._desc_dev = None
        for h, d in responses:
            self.add(h, d)

    def __len__(self):
        return len(self.desc)

    def add(self, h, d: int) -> int:
        h = np.ascontiguousarray(h, dtype=np.float32).reshape(-1)
        K = h.shape[0]
        if not 1 <= K <= MAX_TAPS or not 0 <= int(d) < K:
            raise ValueError(f'a response of K={K} taps with its direct path at {d}: need 1 <= K <= {MAX_TAPS}, 0 <= d < K')
        if 4 * (self._n_taps + K) > MAX_BANK_BYTES:
            raise ValueError(f'the impulse responses need {4 * (self._n_taps + K)} bytes on the device, above the cap of '
                             f'{MAX_BANK_BYTES}: use fewer responses or a smaller rir_max_seconds')
        self.desc = np.concatenate([self.desc, np.array([[self._n_taps, K, int(d)]], dtype=np.int32)])
        self._taps.append(h)
        self._n_taps += K
        self._taps_dev = self._desc_dev = None
        return len(self.desc) - 1

    def response(self, b: int):
        """(h float32 [K], d) of response ``b``, as uploaded"""
        return self._taps[b], int(self.desc[b, 2])

    def device_tables(self, device):
        """(taps fp32 [n_taps], descriptors int32 [n, 3]) on ``device``, uploaded at the first call"""
        import torch
        if self._taps_dev is not None and self._taps_dev.device != device:
            raise RuntimeError('a RirBank belongs to one device')
        if self._taps_dev is None and self._taps:
            self._taps_dev = torch.from_numpy(np.concatenate(self._taps)).to(device)
            self._desc_dev = torch.from_numpy(np.ascontiguousarray(self.desc)).to(device)
        return self._taps_dev, self._desc_dev


def _device_batch(audio):
    import torch
    if not audio.is_cuda or audio.dtype != torch.float32 or not audio.is_contiguous() or audio.dim() != 2:
        raise ValueError('the augmentation kernels want a contiguous fp32 batch [N, L] on the GPU (there is no CPU path)')


def reverb_device(audio, rows: np.ndarray, bank: RirBank):
    """audio fp32 [N, L] on the device; rows int32 [N, 2] = {n_in, response index or -1} -> a new fp32 [N, L]: every row
    convolved with its response over [0, n_in), zero beyond; rows with -1 are copied"""
    import torch
    from .._lib import check, lib, ptr, stream_ptr
    _device_batch(audio)
    rows = np.ascontiguousarray(rows, dtype=np.int32)
    n, L = audio.shape
    if rows.shape != (n, 2):
        raise ValueError(f'{n} rows of audio, a row table of shape {rows.shape}')
    taps, desc_dev = bank.device_tables(audio.device)
    rows_dev = torch.from_numpy(rows).to(audio.device)
    out = torch.empty_like(audio)
    desc = np.ascontiguousarray(bank.desc)
    check(lib.w2l_reverb(ptr(audio), L, ptr(out), L, n, rows.ctypes.data, ptr(rows_dev), desc.ctypes.data if len(desc) else None,
                         ptr(desc_dev), len(desc), ptr(taps), 0 if taps is None else taps.numel(), stream_ptr()), 'w2l_reverb')
    return out


def mix_noise_device(audio, lens, noise, rows: np.ndarray, snr):
    """audio fp32 [N, L] and noise fp32 [N, Z] on the device; lens [N] = n_in per row; rows int32 [N, 2] = {n_z, o} (n_z = 0:
    no noise for this row); snr [N] in dB -> a new fp32 [N, L] with the (wrapped) clip added at exactly that SNR"""
    import torch
    from .._lib import check, lib, ptr, stream_ptr
    _device_batch(audio)
    n, L = audio.shape
    table = np.zeros((n, 3), dtype=np.int32)
    table[:, 0] = np.asarray(lens, dtype=np.int64).reshape(-1)
    table[:, 1:] = np.asarray(rows, dtype=np.int64).reshape(n, 2)
    if noise is None:
        noise = torch.zeros(n, 1, dtype=torch.float32, device=audio.device)
    _device_batch(noise)
    if noise.shape[0] != n:
        raise ValueError(f'{n} rows of audio, {noise.shape[0]} of noise')
    table_dev = torch.from_numpy(table).to(audio.device)
    snr_dev = torch.as_tensor(np.asarray(snr, dtype=np.float32).reshape(n)).to(audio.device)
    n_slab = int(lib.w2l_mix_noise_slab_doubles(n, L))
    slab = torch.empty(max(n_slab, 1), dtype=torch.float64, device=audio.device)
    out = torch.empty_like(audio)
    check(lib.w2l_mix_noise(ptr(audio), L, ptr(noise), noise.shape[1], ptr(out), L, n, table.ctypes.data, ptr(table_dev), ptr(snr_dev),
                            ptr(slab), slab.numel(), stream_ptr()), 'w2l_mix_noise')
    return out


def read_manifest_paths(path) -> List[str]:
    """the ``audio_filepath`` column of a .csv or JSON-lines manifest; ``text`` is not required"""
    path = str(path)
    if path.endswith('.csv'):
        import pandas as pd
        return [str(p) for p in pd.read_csv(path)['audio_filepath']]
    with open(path) as f:
        return [json.loads(line)['audio_filepath'] for line in f if line.strip()]


class RowPlan(NamedTuple):
    """what ``WaveformAugment.draw`` decided for one utterance: the response index or -1; the noise clip index or -1, the
    SNR in dB and the offset as a fraction of the clip (offset = int(frac * n_z) once the clip is read)"""
    rir: int
    clip: int
    snr_db: float
    frac: float


class WaveformAugment:
    """Reverberation and noise for the batches of the train loader.  ``draw(n)`` decides on the host, from a
    ``random.Random`` (as SpecAugment and SpeedPerturb draw); ``apply`` runs the plan on the staged batch.  Per utterance, in
    batch order: u = random(); if u < rir_prob: rir = randrange(n_rirs); u = random(); if u < noise_prob: clip =
    randrange(n_clips), snr = uniform(lo, hi), frac = random().  A side without a manifest is never selected and draws nothing."""

    def __init__(self, noise_manifest=None, rir_manifest=None, noise_prob=0.5, rir_prob=0.5, snr_db=(5, 20), rir_max_seconds=0.5,
                 model_rate=16000, rng=None):
        self.noise_prob, self.rir_prob = float(noise_prob), float(rir_prob)
        for name, v in (('noise_prob', self.noise_prob), ('rir_prob', self.rir_prob)):
            if not 0.0 <= v <= 1.0:
                raise ValueError(f'{name}={v} is no probability')
        self.snr_db = parse_range(snr_db)
        self.rir_max_seconds = float(rir_max_seconds)
        if not self.rir_max_seconds > 0:
            raise ValueError(f'rir_max_seconds={rir_max_seconds} must be positive')
        self.model_rate = int(model_rate)
        self._rng = rng if rng is not None else random.Random()
        self.noise_paths = read_manifest_paths(noise_manifest) if noise_manifest else []
        self.rir_paths = read_manifest_paths(rir_manifest) if rir_manifest else []
        if noise_manifest and not self.noise_paths:
            raise ValueError(f'{noise_manifest} lists no noise clip')
        if rir_manifest and not self.rir_paths:
            raise ValueError(f'{rir_manifest} lists no impulse response')
        self.bank = None
        if self.rir_paths:                               # every response prepared once, here
            from .data_loader import read_audio
            self.bank = RirBank()
            for p in self.rir_paths:
                samples, sr = read_audio(p)
                self.bank.add(*prepare_rir(samples, sr, self.model_rate, self.rir_max_seconds))
        self._resample_banks = None

    @property
    def active(self) -> bool:
        return bool(self.noise_paths or self.rir_paths)

    def draw(self, n: int) -> List[RowPlan]:
        plan = []
        for _ in range(n):
            rir, clip, snr, frac = -1, -1, 0.0, 0.0
            if self.rir_paths:
                if self._rng.random() < self.rir_prob:
                    rir = self._rng.randrange(len(self.rir_paths))
            if self.noise_paths:
                if self._rng.random() < self.noise_prob:
                    clip = self._rng.randrange(len(self.noise_paths))
                    snr = self._rng.uniform(*self.snr_db)
                    frac = self._rng.random()
            plan.append(RowPlan(rir, clip, snr, frac))
        return plan

    __call__ = draw

    def noise_batch(self, plan: Sequence[RowPlan], device):
        """the clips the plan names, read, brought to the model's rate and padded: (noise fp32 [N, Z] on the device or None,
        rows int32 [N, 2] = {n_z, o})"""
        import torch
        from .data_loader import read_audio
        from .resample import BankCache, plan_rows, resample_device
        n = len(plan)
        rows = np.zeros((n, 2), dtype=np.int32)
        picked = [i for i, r in enumerate(plan) if r.clip >= 0]
        if not picked:
            return None, rows
        clips = [read_audio(self.noise_paths[plan[i].clip]) for i in picked]
        lens = [c.shape[0] for c, _ in clips]
        if min(lens) == 0:
            raise ValueError('a noise clip is empty: ' + self.noise_paths[plan[picked[int(np.argmin(lens))]].clip])
        host = torch.zeros(n, max(lens), dtype=torch.float32)
        n_in, rates = np.zeros(n, dtype=np.int64), [self.model_rate] * n
        for i, (c, sr) in zip(picked, clips):
            host[i, :c.shape[0]] = torch.from_numpy(c)
            n_in[i], rates[i] = c.shape[0], sr
        noise = host.to(device)
        if any(sr != self.model_rate for sr in rates):
            if self._resample_banks is None:
                self._resample_banks = BankCache()
            rs = plan_rows(n_in, rates, self.model_rate, None, self._resample_banks)
            noise = resample_device(noise, rs, self._resample_banks)
            n_in = rs[:, 1].astype(np.int64)
        for i in picked:
            rows[i] = (n_in[i], int(plan[i].frac * int(n_in[i])))
        return noise, rows

    def apply(self, audio, lens: np.ndarray, plan: Sequence[RowPlan]):
        """audio fp32 [N, L] on the device with ``lens`` valid samples per row -> the augmented batch (same shape)"""
        if len(plan) != audio.shape[0]:
            raise ValueError(f'{audio.shape[0]} rows of audio, a plan of {len(plan)}')
        if any(r.rir >= 0 for r in plan):
            rows = np.stack([np.asarray(lens, dtype=np.int32), np.array([r.rir for r in plan], dtype=np.int32)], axis=1)
            audio = reverb_device(audio, rows, self.bank)
        if any(r.clip >= 0 for r in plan):
            noise, rows = self.noise_batch(plan, audio.device)
            audio = mix_noise_device(audio, lens, noise, rows, [r.snr_db for r in plan])
        return audio


def from_config(cfg, model_rate: int) -> Optional[WaveformAugment]:
    """the ``data.*`` keys noise_manifest, noise_prob, snr_db, rir_manifest, rir_prob, rir_max_seconds -> a WaveformAugment,
    or None when both manifests are None (off: the loader issues the launches it issues without this module)"""
    def unset(v):
        return v is None or v is False or v == '' or (isinstance(v, str) and v.lower() in ('none', 'null', 'false'))
    noise, rir = cfg.get('noise_manifest'), cfg.get('rir_manifest')
    noise, rir = (None if unset(noise) else noise), (None if unset(rir) else rir)
    check_config(cfg)
    if noise is None and rir is None:
        return None
    return WaveformAugment(noise, rir, cfg.get('noise_prob', 0.5), cfg.get('rir_prob', 0.5), cfg.get('snr_db', (5, 20)),
                           cfg.get('rir_max_seconds', 0.5), model_rate)


def check_config(cfg) -> None:
    """ValueError for a reversed ``snr_db`` range or a probability outside [0, 1], whether or not a manifest is set"""
    parse_range(cfg.get('snr_db', (5, 20)))
    for key in ('noise_prob', 'rir_prob'):
        v = float(cfg.get(key, 0.5))
        if not 0.0 <= v <= 1.0:
            raise ValueError(f'data.{key}={v} is no probability')
