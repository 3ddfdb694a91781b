#!/usr/bin/env python3
"""Timing of the sample-rate converter (w2l_resample) on 32 utterances x 16 s, beside the feature launches it feeds:
HIP-event time per launch with the audio resident, (input + output bytes) / time, and the time of w2l_logmel +
w2l_feature_normalize on the resampled batch, measured as tools/bench_features.py measures them."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from wav2letter_pytorch_amd._lib import check, lib, ptr, stream_ptr  # noqa: E402
from wav2letter_pytorch_amd.data.data_loader import SpectrogramExtractor  # noqa: E402
from wav2letter_pytorch_amd.data.resample import BankCache, plan_rows  # noqa: E402

MODEL_RATE, N, SECONDS = 16000, 32, 16
CASES = [('48 k -> 16 k', 48000, 1), ('44.1 k -> 16 k', 44100, 1), ('8 k -> 16 k', 8000, 1), ('16 k, speed 1.1', 16000, 1.1)]
ext = SpectrogramExtractor(dict(window='hamming', window_stride=0.01, window_size=0.02, sample_rate=MODEL_RATE), 64)


def timed(fn, reps=20):
    for _ in range(3):
        fn()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps * 1e3           # us


for name, rate, speed in CASES:
    L = rate * SECONDS
    banks = BankCache()
    rows = plan_rows([L] * N, [rate] * N, MODEL_RATE, [speed] * N, banks)
    taps, desc_dev = banks.device_tables(torch.device('cuda'))
    rows_dev = torch.from_numpy(rows).cuda()
    desc = np.ascontiguousarray(banks.desc)
    n_out = int(rows[0, 1])
    audio = 0.1 * torch.randn(N, L, device='cuda')
    out = torch.empty(N, n_out, device='cuda')

    def resample():
        check(lib.w2l_resample(ptr(audio), L, ptr(out), n_out, N, rows.ctypes.data, ptr(rows_dev), desc.ctypes.data, ptr(desc_dev),
                               len(desc), ptr(taps), taps.numel(), stream_ptr()), 'w2l_resample')

    noise = torch.randn(N, n_out, device='cuda')
    lens = torch.full((N,), n_out, dtype=torch.int32, device='cuda')
    T = 1 + n_out // ext.hop_length
    mean = torch.empty(N, 64, device='cuda')
    std = torch.empty_like(mean)
    feats = torch.empty(N, 64, T, device='cuda')

    def features():
        lm = ext._launch(out, lens, noise, True, T)
        check(lib.w2l_feature_normalize(ptr(lm), ptr(lens), ext.hop_length, N, T, 64, 1e-5, ptr(mean), ptr(std), ptr(feats), stream_ptr()))

    us = timed(resample)
    us_feat = timed(features)
    nbytes = 4 * N * (L + n_out)
    P, Q, K = int(rows[0, 2]), int(rows[0, 3]), int(banks.desc[0, 1])
    print(f'{name:>16}: ratio {P}/{Q}, K = {K}, bank {4 * Q * K / 1024:.0f} KB; resample {us:.1f} us per launch of {N} x {SECONDS} s, '
          f'{nbytes / 1e6:.1f} MB in + out -> {nbytes / us / 1e3:.0f} GB/s; logmel + normalize on its output {us_feat:.1f} us')
