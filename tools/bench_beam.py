#!/usr/bin/env python3
"""Device CTC prefix beam search (w2l_ctc_beam_search) timing: N=32 utterances, T in {500, 1000}, 29 labels, k in {5, 16, 32}
on peaky, model-like synthetic posteriors; beside it the host decoder (beam_search.prefix_beam_search) on ONE float64
utterance of the same shape.  Device times: CUDA events around back-to-back launches after warm-up (kernel only), and the
wall time of one prefix_beam_search_gpu call (launch, the one copy to the host, the strings).

    python tools/bench_beam.py [--reps 10] [--host-k 5,16,32] [--json PATH]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from wav2letter_pytorch_amd._lib import check, lib, ptr, stream_ptr  # noqa: E402
from wav2letter_pytorch_amd.beam_search import _label_info, prefix_beam_search, prefix_beam_search_gpu  # noqa: E402
from wav2letter_pytorch_amd.data.label_sets import english_labels  # noqa: E402


def peaky(seed, n, t, a, blank=0, boost=(6.0, 12.0), p_blank=0.6, max_burst=3):
    """blank-dominant posteriors with bursts of one character (a trained model's look), float32 [n, t, a]"""
    rng = np.random.default_rng(seed)
    logits = rng.standard_normal((n, t, a))
    for u in range(n):
        f = 0
        while f < t:
            if rng.random() < p_blank:
                logits[u, f, blank] += rng.uniform(*boost)
                f += 1
                continue
            c = int(rng.integers(1, a))
            burst = int(rng.integers(1, max_burst + 1))
            logits[u, f:f + burst, c] += rng.uniform(*boost)
            f += burst
    e = np.exp(logits - logits.max(-1, keepdims=True))
    return (e / e.sum(-1, keepdims=True)).astype(np.float32)


def time_launches(x, k, reps, beta=5.0, prune=1e-3):
    n, t, a = x.shape
    info, end = _label_info(english_labels, 0, '>')
    ws_bytes = int(lib.w2l_ctc_beam_search_workspace_bytes(n, t, k, 0))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=x.device)
    out = torch.empty(12 * n * k + 4 * n + 4 * n * k * t, dtype=torch.uint8, device=x.device)

    def launch():
        check(lib.w2l_ctc_beam_search(ptr(x), None, n, t, a, info.ctypes.data_as(C.c_void_p), 0, end, -1, k, 0.0, beta, prune, 0,
                                      None, 0, None, 0, None, 0.0, ptr(ws), ws_bytes, ptr(out), stream_ptr()),
              'w2l_ctc_beam_search')
    for _ in range(3):
        launch()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        launch()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--host-k', default='5,16,32', help='beam widths at which the host decoder is timed (empty: none)')
    ap.add_argument('--json', default=None)
    args = ap.parse_args()
    host_ks = {int(v) for v in args.host_k.split(',') if v}
    rows = []
    for t in (500, 1000):
        p = peaky(t, 32, t, len(english_labels))
        x = torch.from_numpy(p).cuda()
        passing = float((p > 1e-3).sum(-1).mean())
        for k in (5, 16, 32):
            ms = time_launches(x, k, args.reps)
            torch.cuda.synchronize()
            w0 = time.perf_counter()
            best = prefix_beam_search_gpu(x, english_labels, k=k)
            wall = (time.perf_counter() - w0) * 1e3
            row = dict(N=32, T=t, A=len(english_labels), k=k, labels_per_frame=round(passing, 2), gpu_kernel_ms=round(ms, 3),
                       gpu_call_ms=round(wall, 2), mean_len=round(float(np.mean([len(b) for b in best])), 1))
            if k in host_ks:
                h0 = time.perf_counter()
                ref = prefix_beam_search(p[0].astype(np.float64), english_labels, k=k)
                row['host_one_utt_ms'] = round((time.perf_counter() - h0) * 1e3, 1)
                row['utt0_matches_host'] = ref == best[0]
            rows.append(row)
            print(json.dumps(row), flush=True)
    if args.json:
        with open(args.json, 'w') as f:
            json.dump(rows, f, indent=1)


if __name__ == '__main__':
    main()
