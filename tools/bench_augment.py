#!/usr/bin/env python3
"""Timing of the waveform augmentations (w2l_reverb, w2l_mix_noise) on 32 utterances x 16 s at 16 kHz, audio resident.

Reverberation, K in {2000, 4000, 8000} taps on every row: the shipped Toeplitz / MFMA form and the direct form of
tools/probe/reverb_direct.hip (compiled here into tools/probe/libreverb_direct.so when it is missing), timed INTERLEAVED in
one process -- every round times each candidate once, one HIP event pair per launch -- and, as an outside yardstick, a
torch.fft.rfft convolution of the same batch.  Reported: median [min .. max] over the rounds, achieved TFLOP/s =
2 N L K / time and that as a fraction of the 157.3 TFLOP/s fp32 peak.  The direct form's output is checked against the
shipped form's on the way.

Noise mixing: both launches of w2l_mix_noise, the bytes they move (x and z read twice, one write), and a torch device copy
moving the same number of bytes."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from wav2letter_pytorch_amd._lib import check, lib, ptr, stream_ptr  # noqa: E402
from wav2letter_pytorch_amd.data.augment_wave import RirBank  # noqa: E402

N, SECONDS, RATE, PEAK_TFLOPS = 32, 16, 16000, 157.3
L = SECONDS * RATE
ROUNDS = 15


def direct_form():
    src = os.path.join(ROOT, 'tools', 'probe', 'reverb_direct.hip')
    so = os.path.join(ROOT, 'tools', 'probe', 'libreverb_direct.so')
    if not os.path.exists(so) or os.path.getmtime(so) < os.path.getmtime(src):
        subprocess.run([os.environ.get('HIPCC', '/opt/rocm/bin/hipcc'), '--offload-arch=gfx950', '-O3', '-std=c++17', '-shared', '-fPIC',
                        src, '-o', so], check=True)
    fn = ctypes.CDLL(so).reverb_direct
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p,
                   ctypes.c_void_p, ctypes.c_void_p]
    return fn


def interleaved(fns, rounds=ROUNDS, warmup=3):
    """{name: fn} -> {name: sorted times in us}: each round times every fn once, in turn"""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    pairs = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            fn()
            e.record()
            pairs[k].append((s, e))
    torch.cuda.synchronize()
    return {k: sorted(s.elapsed_time(e) * 1e3 for s, e in v) for k, v in pairs.items()}


def show(ts):
    return f'{ts[len(ts) // 2]:9.1f} us [{ts[0]:.1f} .. {ts[-1]:.1f}]'


def smooth_length(n):
    """the next length >= n whose only prime factors are 2, 3, 5"""
    while True:
        m = n
        for p in (2, 3, 5):
            while m % p == 0:
                m //= p
        if m == 1:
            return n
        n += 1


def main():
    torch.manual_seed(0)
    dev = torch.device('cuda')
    print(f'{torch.cuda.get_device_name(0)}; {N} rows x {SECONDS} s at {RATE} Hz = {N * L} outputs; {ROUNDS} interleaved rounds, median [min .. max]')
    audio = 0.1 * torch.randn(N, L, device=dev)
    out = torch.empty_like(audio)
    out2 = torch.empty_like(audio)
    direct = direct_form()
    print('-- w2l_reverb')
    for K in (2000, 4000, 8000):
        g = np.random.default_rng(K)
        bank = RirBank([((g.standard_normal(K) * np.exp(-np.arange(K) / (K / 6.0))).astype(np.float32), 40) for _ in range(4)])
        rows = np.array([(L, n % 4) for n in range(N)], dtype=np.int32)
        taps, desc_dev = bank.device_tables(dev)
        rows_dev = torch.from_numpy(rows).to(dev)
        desc = np.ascontiguousarray(bank.desc)

        def shipped():
            check(lib.w2l_reverb(ptr(audio), L, ptr(out), L, N, rows.ctypes.data, ptr(rows_dev), desc.ctypes.data, ptr(desc_dev), len(desc),
                                 ptr(taps), taps.numel(), stream_ptr()), 'w2l_reverb')

        def probe():
            rc = direct(ptr(audio), L, ptr(out2), L, N, ptr(rows_dev), ptr(desc_dev), ptr(taps), stream_ptr())
            assert rc == 0, rc

        nfft = smooth_length(L + K - 1)
        hpad = torch.zeros(N, nfft, device=dev)
        for n in range(N):
            hpad[n, :K] = taps[int(desc[n % 4, 0]):int(desc[n % 4, 0]) + K]
        hf = torch.fft.rfft(hpad)                        # the responses' spectra are formed once, as a bank would hold them

        def fft():
            return torch.fft.irfft(torch.fft.rfft(audio, n=nfft) * hf, n=nfft)[:, 40:40 + L]

        shipped()
        probe()
        yf = fft()
        torch.cuda.synchronize()
        scale = float(out.abs().max())
        print(f'K = {K}: direct form differs from the shipped form by at most {float((out - out2).abs().max()) / scale:.2e} of the peak, '
              f'the rfft convolution (n = {nfft}) by {float((out - yf).abs().max()) / scale:.2e}')
        ts = interleaved({'toeplitz mfma (shipped)': shipped, 'direct valu (probe)': probe, 'torch rfft yardstick': fft})
        flop = 2.0 * N * L * K
        for name, t in ts.items():
            med = t[len(t) // 2]
            extra = '' if 'rfft' in name else f'  {flop / med / 1e6:6.1f} TFLOP/s = {100 * flop / med / 1e6 / PEAK_TFLOPS:4.1f} % of {PEAK_TFLOPS}'
            print(f'   {name:>24}: {show(t)}{extra}')

    print('-- w2l_mix_noise')
    noise = 0.1 * torch.randn(N, L, device=dev)
    table = np.array([(L, L, 1234)] * N, dtype=np.int32)
    table_dev = torch.from_numpy(table).to(dev)
    snr = torch.full((N,), 10.0, device=dev)
    slab = torch.empty(int(lib.w2l_mix_noise_slab_doubles(N, L)), dtype=torch.float64, device=dev)
    moved = 5 * 4 * N * L                                # x and z read by both passes, one write
    src = torch.empty(moved // 8, device=dev)
    dst = torch.empty_like(src)

    def mix():
        check(lib.w2l_mix_noise(ptr(audio), L, ptr(noise), L, ptr(out), L, N, table.ctypes.data, ptr(table_dev), ptr(snr), ptr(slab),
                                slab.numel(), stream_ptr()), 'w2l_mix_noise')

    ts = interleaved({'power + apply': mix, 'torch copy, same bytes': lambda: dst.copy_(src)})
    for name, t in ts.items():
        med = t[len(t) // 2]
        print(f'   {name:>24}: {show(t)}  {moved / 1e6:.0f} MB moved -> {moved / med / 1e3:.0f} GB/s')


if __name__ == '__main__':
    main()
