#!/usr/bin/env python3
"""CTC keyword search (w2l_ctc_kws) timing: N=32 utterances, T=500, 29 labels, K in {1, 32, 256} keywords of 4-12 labels on random
log-softmax frames.  Per K: the whole call's three launches and each launch alone (the entry point's ``phases`` mask: frame
maxima, scan, pick), and in the same process, taken alternately with them round by round, w2l_ctc_align on the same N and T with
one target per utterance whose 2 S + 1 states fill the scan's block width -- the same sequential depth, one barrier per frame,
so it is the yardstick of the scan's per-frame cost.  Medians over --rounds rounds of --reps back-to-back launches between
events; then the wall time of one ctc_keyword_search call (launches, copies to the host, the hit lists).

    python tools/bench_kws.py [--reps 20] [--rounds 7] [--json PATH]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from wav2letter_pytorch_amd.alignment import align_sections, launch_align  # noqa: E402
from wav2letter_pytorch_amd.keyword_search import KeywordTable, ctc_keyword_search, kws_sections, launch_kws  # noqa: E402


def window(launch, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        launch()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--json', default=None)
    args = ap.parse_args()
    n, t, a, max_hits = 32, 500, 29, 8
    rng = np.random.default_rng(0)
    x = torch.randn(n, t, a, generator=torch.Generator().manual_seed(t)).mul(2).log_softmax(-1).cuda()
    rows = []
    for k in (1, 32, 256):
        kws = [rng.integers(1, a, int(s)).tolist() for s in rng.integers(4, 13, k)]
        table = KeywordTable(kws)
        chunk = table.chunks[0]
        width = chunk['width']
        _, dev_table = table.on_device(0, x.device)
        thr = torch.from_numpy(-1.0 * table.lengths.astype(np.float32)).cuda()
        small = torch.empty(kws_sections(n, k, max_hits)[3], dtype=torch.uint8, device='cuda')
        score = torch.empty(n, k, t, device='cuda')
        start = torch.empty(n, k, t, dtype=torch.int32, device='cuda')
        ws = launch_kws(x, None, dev_table, thr, max_hits, 0, True, small, score, start)
        # the yardstick: one target per utterance whose 2 S + 1 states fill the same block width
        s_al = (width - 1) // 2
        tg = torch.from_numpy(rng.integers(1, a, (n, s_al)).astype(np.int32)).cuda()
        tl = torch.full((n,), s_al, dtype=torch.int32, device='cuda')
        out = torch.empty(align_sections(n, t, s_al)[5], dtype=torch.uint8, device='cuda')
        keep = []
        runs = {
            'kws_all_ms': lambda: launch_kws(x, None, dev_table, thr, max_hits, 0, True, small, score, start, 7, ws),
            'kws_frame_max_ms': lambda: launch_kws(x, None, dev_table, thr, max_hits, 0, True, small, score, start, 1, ws),
            'kws_scan_ms': lambda: launch_kws(x, None, dev_table, thr, max_hits, 0, True, small, score, start, 2, ws),
            'kws_pick_ms': lambda: launch_kws(x, None, dev_table, thr, max_hits, 0, True, small, score, start, 4, ws),
            'align_ms': lambda: keep.append(launch_align(x, None, tg.data_ptr(), s_al, tl.data_ptr(), 1, s_al, 0, True, out, 0)),
        }
        for run in runs.values():                          # warm-up: code objects, allocator
            for _ in range(3):
                run()
        torch.cuda.synchronize()
        samples = {name: [] for name in runs}
        for _ in range(args.rounds):                       # alternately: drift lands on all of them
            for name, run in runs.items():
                samples[name].append(window(run, args.reps))
            del keep[:]
        torch.cuda.synchronize()
        w0 = time.perf_counter()
        found = ctc_keyword_search(x, table, log_probs=True, max_hits=max_hits)
        wall = (time.perf_counter() - w0) * 1e3
        row = dict(N=n, T=t, A=a, K=k, states=int((chunk['meta'] >= 0).sum()), width=width, blocks=chunk['n_blocks'],
                   align_states=2 * s_al + 1)
        for name, v in samples.items():
            row[name] = round(statistics.median(v), 4)
            row[name.replace('_ms', '_spread')] = round((max(v) - min(v)) / statistics.median(v), 3)
        row['scan_over_align'] = round(row['kws_scan_ms'] / row['align_ms'], 3)
        row['scan_us_per_frame'] = round(1e3 * row['kws_scan_ms'] / t, 4)
        row['align_us_per_frame'] = round(1e3 * row['align_ms'] / t, 4)
        row['search_call_ms'] = round(wall, 2)
        row['hits'] = sum(len(f) for f in found)
        rows.append(row)
        print(json.dumps(row), flush=True)
    if args.json:
        with open(args.json, 'w') as f:
            json.dump(rows, f, indent=1)


if __name__ == '__main__':
    main()
