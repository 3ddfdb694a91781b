#!/usr/bin/env python3
"""Wildcard CTC kernel timing at the headline loss shape (N=32, T'=500, C=29, targets as bench.py draws them:
defaults.synthetic_batch(32, 1000, seed=1234), 80..160 labels): w2l_ctc_loss -- the yardstick, twice, so that the spread between
two runs of one kernel is on the page -- and w2l_wctc_loss on the same rows without stars, with a star at both ends, and with a
star in every gap.  A row with a star in every gap is 2 S + 1 entries wide, and the block width follows the raw row width (the
labels are counted on the device, the host never reads them): that variant runs on a wider block than CTC does, so the same
pattern is also timed on transcripts cut to half, whose raw rows are as wide as the CTC rows.  All are timed in interleaved
rounds in one process (device events around REPS back-to-back calls each), loss + gradient, median and minimum over the rounds.

    python tools/bench_wctc.py [--rounds 15] [--reps 20] > profiles/wctc_bench.txt
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from wav2letter_pytorch_amd._lib import check, lib, ptr, stream_ptr  # noqa: E402
from wav2letter_pytorch_amd.defaults import synthetic_batch  # noqa: E402

N, T, C = 32, 500, 29
STAR = C
KWIDE = (64, 128, 192, 256, 320, 384, 448, 512, 640, 768, 896, 1024)


def padded(rows):
    tl = torch.tensor([len(r) for r in rows], dtype=torch.int32)
    tg = torch.zeros(len(rows), int(tl.max()), dtype=torch.int32)
    for n, r in enumerate(rows):
        tg[n, :len(r)] = torch.tensor(r, dtype=torch.int32)
    return tg.cuda(), tl.cuda()


def every_gap(z):
    row = [STAR]
    for v in z:
        row += [v, STAR]
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=15)
    ap.add_argument('--reps', type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_wctc.py measures on the GPU: no device found')
    _, _, tg, tl = synthetic_batch(N, 2 * T, seed=1234)
    rows = [tg[n, :int(tl[n])].tolist() for n in range(N)]
    gen = torch.Generator().manual_seed(0)
    xd = torch.log_softmax(torch.randn(N, T, C, generator=gen) * 2, -1).cuda()
    ild = torch.full((N,), T, dtype=torch.int32).cuda()
    variants = {
        'w2l_ctc_loss': rows,
        'w2l_wctc_loss, no stars': rows,
        'w2l_wctc_loss, stars at both ends': [[STAR] + r + [STAR] for r in rows],
        'w2l_wctc_loss, stars in every gap': [every_gap(r) for r in rows],
        'w2l_wctc_loss, stars in every gap, half the labels': [every_gap(r[:(len(r) - 1) // 2]) for r in rows],
        'w2l_ctc_loss (again)': rows,
    }
    nll = torch.empty(N, device='cuda')
    loss = torch.empty(1, device='cuda')
    status = torch.empty(N, dtype=torch.int32, device='cuda')
    grad = torch.empty(N, T, C, device='cuda')
    runs, info = {}, {}
    for name, r in variants.items():
        tgd, tld = padded(r)
        smax = tgd.shape[1]
        wild = 'wctc' in name
        nbytes = (lib.w2l_wctc_workspace_bytes if wild else lib.w2l_ctc_workspace_bytes)(N, T, smax)
        ws = torch.empty(int(nbytes), dtype=torch.uint8, device='cuda')

        def call(tgd=tgd, tld=tld, smax=smax, ws=ws, wild=wild):
            if wild:
                check(lib.w2l_wctc_loss(ptr(xd), ptr(tgd), ptr(ild), ptr(tld), N, T, C, smax, 0, 1, STAR, 0.0, ptr(nll), ptr(loss),
                                        ptr(grad), ptr(status), ptr(ws), stream_ptr()), 'w2l_wctc_loss')
            else:
                check(lib.w2l_ctc_loss(ptr(xd), ptr(tgd), ptr(ild), ptr(tld), N, T, C, smax, 0, 1, ptr(nll), ptr(loss), ptr(grad),
                                       ptr(ws), stream_ptr()), 'w2l_ctc_loss')

        runs[name] = call
        call()
        torch.cuda.synchronize()
        width = next((w for w in KWIDE if 2 * smax + 1 <= w), 1024)
        info[name] = (smax, width, float(loss[0]), int((status != 0).sum()) if wild else 0)
    print(f'shape: N={N} T\'={T} C={C}, targets of defaults.synthetic_batch({N}, {2 * T}, seed=1234): {int(tl.min())}..{int(tl.max())} '
          f'labels; loss + gradient, zero_infinity, penalty 0')
    for fn in runs.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in runs}
    for _ in range(args.rounds):
        for name, fn in runs.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(args.reps):
                fn()
            e.record()
            torch.cuda.synchronize()
            times[name].append(s.elapsed_time(e) / args.reps * 1e3)
    base = statistics.median(times['w2l_ctc_loss'])
    for name, v in times.items():
        smax, width, lv, bad = info[name]
        print(f'{name}: median {statistics.median(v):.1f} us, min {min(v):.1f} us per call, {statistics.median(v) / base:.3f}x '
              f'w2l_ctc_loss   (row width {smax}, block {width} threads, loss {lv:.4f}, rows with status != 0: {bad}; '
              f'{args.rounds} interleaved rounds x {args.reps} calls)')


if __name__ == '__main__':
    main()
