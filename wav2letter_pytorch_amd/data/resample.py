"""Band-limited sample-rate conversion and speed perturbation of a batch of waveforms on the GPU (csrc/resample.hip),
the step in front of the log-mel front end for audio that is not at the model's rate.  No reference counterpart: the
reference asserts the rate of the first manifest row (data_loader.py:136-139) and augments spectrograms only.

The arithmetic, for a row of ``n_in`` samples and a reduced ratio ``P/Q`` = input samples advanced per output sample
(``P/Q = speed * file_rate / model_rate``):

    n_out  = ceil(n_in * Q / P)
    out[m] = sum_{j < K} x~[i0 - H + j] * h[phase][j],   i0 = (m P) div Q,  phase = (m P) mod Q   (exact integers)

with ``x~`` zero outside ``[0, n_in)``.  ``h[Q][K]`` is a Kaiser-windowed sinc, built here in float64 and rounded once to
fp32:  c = rolloff * min(1, Q/P),  W = zeros / c,  H = ceil(W),  K = 2H + 2,  u = (j - H) - p/Q,

    h[p][j] = c * sinc(c u) * I0(beta * sqrt(1 - (u/W)^2)) / I0(beta)   for |u| < W, else 0.

Rows with P == Q are copied bit for bit (the filter is a 0.92-Nyquist low-pass, not an identity).  This module imports
without a GPU; only ``resample_batch`` / ``BankCache.device_tables`` touch the device.
"""
from __future__ import annotations

import math
import random
from fractions import Fraction
from typing import Dict, Optional, Sequence, Tuple

import numpy as np

ZEROS, BETA, ROLLOFF = 16, 9.0, 0.92
MAX_BANK_BYTES = 8 << 20         # a larger filter bank is refused (ValueError naming the ratio)
MAX_K = 512                      # W2L_RESAMPLE_MAX_K, W2L_RESAMPLE_MAX_SPAN, W2L_RESAMPLE_TILE (include/w2l_hip.h)
MAX_SPAN = 8192
TILE = 512


def speed_fraction(speed) -> Fraction:
    """a speed factor as the exact ratio used everywhere: 0.9 -> 9/10, 1.1 -> 11/10"""
    if isinstance(speed, Fraction):
        return speed
    return Fraction(str(speed)).limit_denominator(1000)


def resample_ratio(file_rate, model_rate, speed=1) -> Fraction:
    """P/Q = speed * file_rate / model_rate, reduced: input samples advanced per output sample"""
    file_rate, model_rate = int(file_rate), int(model_rate)
    if file_rate <= 0 or model_rate <= 0:
        raise ValueError(f'sample rates must be positive: {file_rate} -> {model_rate}')
    r = speed_fraction(speed) * Fraction(file_rate, model_rate)
    if r <= 0:
        raise ValueError(f'speed factor {speed} is not positive')
    return r


def output_length(n_in: int, ratio: Fraction) -> int:
    """n_out = ceil(n_in * Q / P)"""
    P, Q = ratio.numerator, ratio.denominator
    return -((-int(n_in) * Q) // P)


def bank_shape(P: int, Q: int, zeros=ZEROS, rolloff=ROLLOFF) -> Tuple[int, int]:
    """(K, H) of the bank of ratio P/Q"""
    c = rolloff * min(1.0, Q / P)
    H = int(math.ceil(zeros / c))
    return 2 * H + 2, H


def filter_bank(P: int, Q: int, zeros=ZEROS, beta=BETA, rolloff=ROLLOFF):
    """(float32 [Q, K], H): the polyphase Kaiser-windowed sinc of ratio P/Q, formed in float64 and rounded once"""
    P, Q = int(P), int(Q)
    if P <= 0 or Q <= 0:
        raise ValueError(f'ratio {P}/{Q} is not positive')
    K, H = bank_shape(P, Q, zeros, rolloff)
    if 4 * Q * K > MAX_BANK_BYTES:
        raise ValueError(f'the filter bank of the ratio {P}/{Q} has {Q} phases x {K} taps = {4 * Q * K} bytes, above the cap of '
                         f'{MAX_BANK_BYTES}: resample to a rate with a simpler ratio first')
    c = rolloff * min(1.0, Q / P)
    W = zeros / c
    u = (np.arange(K, dtype=np.float64)[None, :] - H) - np.arange(Q, dtype=np.float64)[:, None] / Q
    inside = np.abs(u) < W
    t = np.where(inside, u / W, 0.0)
    h = c * np.sinc(c * u) * np.i0(beta * np.sqrt(1.0 - t * t)) / np.i0(beta)
    return np.where(inside, h, 0.0).astype(np.float32), H


def parse_speed_factors(value):
    """the ``data.speed_perturb`` config key: None / '' / false -> None; '0.9,1.0,1.1', a list or one number -> a tuple"""
    if value is None or value is False or value == '' or (isinstance(value, str) and value.lower() in ('none', 'null', 'false')):
        return None
    if isinstance(value, str):
        value = [v for v in value.replace('[', '').replace(']', '').split(',') if v.strip()]
    elif isinstance(value, (int, float)):
        value = [value]
    return tuple(float(v) for v in value)


class SpeedPerturb:
    """One speed factor per utterance from ``factors``, drawn on the host from a ``random.Random`` (as SpecAugment draws its
    masks).  The factor is applied on the waveform by the resampler: speed 1.1 shortens the utterance by 1/1.1."""

    def __init__(self, factors=(0.9, 1.0, 1.1), rng=None):
        self.factors = tuple(float(f) for f in factors)
        if not self.factors or any(f <= 0 for f in self.factors):
            raise ValueError(f'speed factors must be positive: {factors!r}')
        self._rng = rng if rng is not None else random.Random()

    def draw(self, n: int):
        return [self.factors[self._rng.randrange(len(self.factors))] for _ in range(n)]

    __call__ = draw


class BankCache:
    """The filter banks of the ratios seen so far, keyed by (P, Q): built once on the host, uploaded once, kept concatenated
    on the device with their descriptor table {offset, K, H, Q} (what w2l_resample reads)."""

    def __init__(self):
        self.index: Dict[Tuple[int, int], int] = {}
        self.desc = np.zeros((0, 4), dtype=np.int32)
        self._n_taps = 0
        self._taps_dev = None
        self._desc_dev = None
        self._pending = []

    def bank(self, P: int, Q: int) -> int:
        key = (int(P), int(Q))
        b = self.index.get(key)
        if b is None:
            K, H = bank_shape(*key)
            if K > MAX_K or ((Q - 1) + (TILE - 1) * P) // Q + K + 6 > MAX_SPAN:
                raise ValueError(f'the ratio {P}/{Q} needs {K} filter taps per output: ratios above about 14 are not supported')
            h, H = filter_bank(*key)
            b = self.index[key] = len(self.index)
            self.desc = np.concatenate([self.desc, np.array([[self._n_taps, K, H, Q]], dtype=np.int32)])
            self._n_taps += h.size
            self._pending.append(h.reshape(-1))
            self._desc_dev = None
        return b

    def device_tables(self, device):
        """(taps fp32 [n_taps], descriptors int32 [n_banks, 4]) on ``device``; only banks added since the last call are uploaded"""
        import torch
        if self._taps_dev is not None and self._taps_dev.device != device:
            raise RuntimeError('a BankCache belongs to one device')
        if self._pending:
            new = torch.from_numpy(np.concatenate(self._pending)).to(device)
            self._taps_dev = new if self._taps_dev is None else torch.cat([self._taps_dev, new])
            self._pending = []
        if self._desc_dev is None and len(self.desc):
            self._desc_dev = torch.from_numpy(self.desc).to(device)
        return self._taps_dev, self._desc_dev


def plan_rows(lengths: Sequence[int], rates: Sequence[int], model_rate: int, speeds, banks: BankCache) -> np.ndarray:
    """the row table of w2l_resample, int32 [N, 5] = {n_in, n_out, P, Q, bank}; bank = -1 for rows that are copied"""
    n = len(lengths)
    rates = [model_rate] * n if rates is None else list(rates)
    speeds = [1] * n if speeds is None else list(speeds)
    if len(rates) != n or len(speeds) != n:
        raise ValueError(f'{n} signals, {len(rates)} rates, {len(speeds)} speeds')
    rows = np.zeros((n, 5), dtype=np.int32)
    for i, (L, fr, sp) in enumerate(zip(lengths, rates, speeds)):
        r = resample_ratio(fr, model_rate, sp)
        P, Q = r.numerator, r.denominator
        rows[i] = (L, output_length(L, r), P, Q, -1 if P == Q else banks.bank(P, Q))
    return rows


def resample_device(audio, rows: np.ndarray, banks: BankCache):
    """audio fp32 [N, L] on the device (row n valid up to rows[n, 0]) -> fp32 [N, max n_out], zero past each row's n_out"""
    import torch
    from .._lib import check, lib, ptr, stream_ptr
    if not audio.is_cuda or audio.dtype != torch.float32 or not audio.is_contiguous():
        raise ValueError('resample_device wants a contiguous fp32 batch on the GPU (there is no CPU path)')
    rows = np.ascontiguousarray(rows, dtype=np.int32)
    n = audio.shape[0]
    taps, desc_dev = banks.device_tables(audio.device)
    rows_dev = torch.from_numpy(rows).to(audio.device)
    out = torch.empty(n, max(1, int(rows[:, 1].max())), dtype=torch.float32, device=audio.device)
    desc = np.ascontiguousarray(banks.desc)
    check(lib.w2l_resample(ptr(audio), audio.shape[1], ptr(out), out.shape[1], n, rows.ctypes.data, ptr(rows_dev),
                           desc.ctypes.data if len(desc) else None, ptr(desc_dev), len(desc), ptr(taps),
                           0 if taps is None else taps.numel(), stream_ptr()), 'w2l_resample')
    return out


_DEFAULT_BANKS: Dict[str, BankCache] = {}


def resample_batch(signals: Sequence, rates: Sequence[int], model_rate: int, speeds: Optional[Sequence] = None, device=None):
    """signals: N 1-D float arrays; rates: their sample rates; speeds: optional speed factors.  Returns (audio fp32
    [N, max n_out] on the device, zero past each row's end; n_out int32 [N] on the host)."""
    import torch
    if device is None:
        if not torch.cuda.is_available():
            raise RuntimeError('resample_batch runs on MI355X only (HIP kernel, no CPU path)')
        device = torch.device('cuda', torch.cuda.current_device())
    device = torch.device(device)
    banks = _DEFAULT_BANKS.setdefault(str(device), BankCache())
    arrs = [np.asarray(s.detach().cpu() if torch.is_tensor(s) else s, dtype=np.float32).reshape(-1) for s in signals]
    rows = plan_rows([a.shape[0] for a in arrs], rates, model_rate, speeds, banks)
    host = torch.zeros(len(arrs), max(1, max(a.shape[0] for a in arrs)), dtype=torch.float32)
    for i, a in enumerate(arrs):
        host[i, :a.shape[0]] = torch.from_numpy(a)
    out = resample_device(host.to(device), rows, banks)
    return out, torch.from_numpy(rows[:, 1].copy())
