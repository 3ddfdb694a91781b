#!/usr/bin/env python3
"""CTC forced alignment (w2l_ctc_align) timing: N=32 utterances, 29 labels, T in {500, 1000}, targets of S in {50, 150} labels on
random log-softmax frames.  Per shape: the align kernel (events around back-to-back launches after warm-up), w2l_ctc_loss
with its gradient at the same (N, T, S) in the same process (the sum-form sibling, a yardstick), the wall time of one
ctc_forced_align call (launch, the one copy to the host), and the host model (alignment.viterbi_align_host, float32) on ONE
utterance.  Then the beam decoder at k in {5, 16} on peaky posteriors: decode(return_offsets=True) against decode(), medians
over --calls calls taken alternately, and their difference.

    python tools/bench_align.py [--reps 20] [--calls 20] [--json PATH]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from wav2letter_pytorch_amd._lib import check, lib, ptr, stream_ptr  # noqa: E402
from wav2letter_pytorch_amd.alignment import align_sections, ctc_forced_align, launch_align, viterbi_align_host  # noqa: E402
from wav2letter_pytorch_amd.beam_search import GPUPrefixBeamSearchDecoder  # noqa: E402
from wav2letter_pytorch_amd.data.label_sets import english_labels  # noqa: E402
from tools.bench_beam import peaky  # noqa: E402


def timed(launch, reps):
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
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--json', default=None)
    args = ap.parse_args()
    n, a = 32, len(english_labels)
    rng = np.random.default_rng(0)
    rows = []
    for t in (500, 1000):
        lp = torch.randn(n, t, a, generator=torch.Generator().manual_seed(t)).mul(2).log_softmax(-1)
        x = lp.cuda()
        for s in (50, 150):
            tg_host = rng.integers(1, a, (n, s)).astype(np.int32)
            tg = torch.from_numpy(tg_host).cuda()
            tl = torch.full((n,), s, dtype=torch.int32, device='cuda')
            il = torch.full((n,), t, dtype=torch.int32, device='cuda')
            out = torch.empty(align_sections(n, t, s)[5], dtype=torch.uint8, device='cuda')
            keep = []
            align_ms = timed(lambda: keep.append(launch_align(x, None, tg.data_ptr(), s, tl.data_ptr(), 1, s, 0, True, out, 0)),
                             args.reps)
            ws = torch.empty(int(lib.w2l_ctc_workspace_bytes(n, t, s)), dtype=torch.uint8, device='cuda')
            nll, loss = torch.empty(n, device='cuda'), torch.empty(1, device='cuda')
            grad = torch.empty_like(x)
            loss_ms = timed(lambda: check(lib.w2l_ctc_loss(ptr(x), ptr(tg), ptr(il), ptr(tl), n, t, a, s, 0, 1, ptr(nll), ptr(loss),
                                                           ptr(grad), ptr(ws), stream_ptr()), 'w2l_ctc_loss'), args.reps)
            fwd_ms = timed(lambda: check(lib.w2l_ctc_loss(ptr(x), ptr(tg), ptr(il), ptr(tl), n, t, a, s, 0, 1, ptr(nll), ptr(loss),
                                                          None, ptr(ws), stream_ptr()), 'w2l_ctc_loss'), args.reps)
            torch.cuda.synchronize()
            w0 = time.perf_counter()
            res = ctc_forced_align(x, tg_host)
            wall = (time.perf_counter() - w0) * 1e3
            h0 = time.perf_counter()
            ref = viterbi_align_host(lp[0].numpy(), tg_host[0], dtype=np.float32)
            host = (time.perf_counter() - h0) * 1e3
            row = dict(N=n, T=t, A=a, S=s, align_kernel_ms=round(align_ms, 4), ctc_loss_grad_ms=round(loss_ms, 4),
                       ctc_loss_fwd_ms=round(fwd_ms, 4), align_call_ms=round(wall, 2), host_one_utt_ms=round(host, 1),
                       utt0_matches_host=bool(np.array_equal(res.paths[0], ref.path)
                                              and np.float32(res.scores[0]).tobytes() == np.float32(ref.score).tobytes()))
            rows.append(row)
            print(json.dumps(row), flush=True)
    for t in (500, 1000):
        p = torch.from_numpy(peaky(t, n, t, a)).cuda()
        for k in (5, 16):
            dec = GPUPrefixBeamSearchDecoder(None, english_labels, k=k)
            for _ in range(3):
                dec.decode(p)
                dec.decode(p, return_offsets=True)
            plain, offs = [], []
            for _ in range(args.calls):                    # alternately: drift lands on both
                for bucket, flag in ((plain, False), (offs, True)):
                    torch.cuda.synchronize()
                    w0 = time.perf_counter()
                    dec.decode(p, return_offsets=flag)
                    bucket.append((time.perf_counter() - w0) * 1e3)
            row = dict(N=n, T=t, A=a, k=k, calls=args.calls, decode_ms=round(statistics.median(plain), 3),
                       decode_offsets_ms=round(statistics.median(offs), 3),
                       added_ms=round(statistics.median(offs) - statistics.median(plain), 3))
            rows.append(row)
            print(json.dumps(row), flush=True)
    if args.json:
        with open(args.json, 'w') as f:
            json.dump(rows, f, indent=1)


if __name__ == '__main__':
    main()
