#!/usr/bin/env python3
"""Long CTC forced alignment (w2l_ctc_align_long) timing on random log-softmax frames, 29 labels, one process.

(a) T = 32768, S = 4095, the one shape w2l_ctc_align and w2l_ctc_align_long both take at the former's limits: the two on the
    same posteriors, launched alternately (old, new, old, new, ...), each launch between device events; medians.  The outputs
    are compared first: they must be the same bytes.
(b) T x S in {(65536, 12000), (120000, 30000), (180000, 50000)} (the last: an hour of audio with its text) for every candidate
    (tb, sb) of alignment.LONG_CANDIDATES, the candidates taken in turn inside every round: the whole call, and the forward
    launches (memset, init, one launch per time block), the back-trace and the output kernel on their own
    (w2l_ctc_align_long_phases, each with the others' results in the workspace).  The pair with the least whole-call median at
    the largest shape is the library's default plan (W2L_ALIGN_LONG_TB / _SB).

    python tools/bench_align_long.py [--rounds 5] [--json PATH] [--small]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from wav2letter_pytorch_amd._lib import check, lib, ptr, stream_ptr  # noqa: E402
from wav2letter_pytorch_amd import alignment as AL  # noqa: E402


def event_ms(launch):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    launch()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e)


def inputs(t, s, a, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(t, a, generator=g).mul(2).log_softmax(-1).cuda().contiguous()
    tg = torch.randint(1, a, (s,), generator=g, dtype=torch.int32).cuda()
    return x, tg


class Long:
    """one (T, S, plan): its workspace and outputs, and launches by phase mask"""

    def __init__(self, x, tg, plan):
        self.x, self.tg, self.plan = x, tg, plan
        t, s = x.shape[0], tg.numel()
        self.ws = torch.empty(AL.long_workspace_bytes(t, s, *plan), dtype=torch.uint8, device='cuda')
        self.out = torch.empty(AL.align_sections(1, t, s)[5], dtype=torch.uint8, device='cuda')

    def launch(self, phases=7):
        t, a = self.x.shape
        s = self.tg.numel()
        vp = C.c_void_p
        sec = [vp(self.out.data_ptr() + o) for o in AL.align_sections(1, t, s)[:5]]
        check(lib.w2l_ctc_align_long_phases(ptr(self.x), t, a, ptr(self.tg), s, 0, 1, self.plan[0], self.plan[1], phases, ptr(self.ws),
                                            int(self.ws.numel()), *sec, stream_ptr()), 'w2l_ctc_align_long_phases')


def med(v):
    return round(statistics.median(v), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--json', default=None)
    ap.add_argument('--small', action='store_true', help='a rehearsal at toy shapes (its numbers mean nothing)')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_align_long needs the MI355X (no CPU path)')
    a = 29
    rows = []

    # ---- (a) both kernels at w2l_ctc_align's limits
    t, s = (2048, 300) if args.small else (32768, 4095)
    x, tg = inputs(t, s, a, 1)
    tl = torch.full((1,), s, dtype=torch.int32, device='cuda')
    x3 = x.view(1, t, a)
    old_out = torch.empty(AL.align_sections(1, t, s)[5], dtype=torch.uint8, device='cuda')
    keep = []

    def old():
        keep[:] = [AL.launch_align(x3, None, tg.data_ptr(), max(s, 1), tl.data_ptr(), 1, s, 0, True, old_out, 0)]

    legs = {'w2l_ctc_align': old}
    news = {}
    for plan in AL.LONG_CANDIDATES:
        news[plan] = Long(x, tg, plan)
        legs['long tb=%d sb=%d' % plan] = news[plan].launch
    for f in legs.values():                                # warm-up, and the results that must agree
        f()
        f()
    torch.cuda.synchronize()
    want = old_out.cpu().numpy()
    same = all(np.array_equal(want, n.out.cpu().numpy()) for n in news.values())
    times = {k: [] for k in legs}
    for _ in range(args.rounds):
        for k, f in legs.items():
            times[k].append(event_ms(f))
    for k, v in times.items():
        row = dict(part='a', T=t, S=s, leg=k, ms_median=med(v), ms_min=round(min(v), 3), ms_max=round(max(v), 3), rounds=args.rounds,
                   outputs_equal_old=bool(same))
        rows.append(row)
        print(json.dumps(row), flush=True)
    del news, legs, keep, old_out

    # ---- (b) the candidates at long shapes
    shapes = [(4096, 1000), (6000, 2500)] if args.small else [(65536, 12000), (120000, 30000), (180000, 50000)]
    for t, s in shapes:
        x, tg = inputs(t, s, a, t)
        runs = [Long(x, tg, plan) for plan in AL.LONG_CANDIDATES]
        ref = None
        for r in runs:
            r.launch()
            r.launch()
            torch.cuda.synchronize()
            got = r.out.cpu().numpy()
            ref = got if ref is None else ref
            assert np.array_equal(ref, got), ('the plans disagree', r.plan)
        parts = {r.plan: {m: [] for m in (7, 1, 2, 4)} for r in runs}
        for _ in range(args.rounds):
            for r in runs:
                for m in (7, 1, 2, 4):
                    parts[r.plan][m].append(event_ms(lambda: r.launch(m)))
        for r in runs:
            p = parts[r.plan]
            nt, spt = (lambda w: (-(-w // (64 * (1 if w <= 1024 else 2 if w <= 2048 else 4))) * 64, 1 if w <= 1024 else 2 if w <= 2048 else 4))(
                r.plan[1] + 2 * r.plan[0])
            row = dict(part='b', T=t, S=s, tb=r.plan[0], sb=r.plan[1], threads=nt, states_per_thread=spt, launches=-(-t // r.plan[0]),
                       tiles=-(-(2 * s + 1) // r.plan[1]), workspace_GB=round(r.ws.numel() / 1e9, 3), total_ms=med(p[7]),
                       total_min=round(min(p[7]), 3), total_max=round(max(p[7]), 3), forward_ms=med(p[1]), backtrace_ms=med(p[2]),
                       output_ms=med(p[4]), rounds=args.rounds)
            rows.append(row)
            print(json.dumps(row), flush=True)
        best = min(runs, key=lambda r: statistics.median(parts[r.plan][7]))
        print(json.dumps(dict(part='b', T=t, S=s, winner=list(best.plan), library_default=list(AL.LONG_PLAN))), flush=True)
        del runs, parts
        torch.cuda.empty_cache()
    if args.json:
        with open(args.json, 'w') as f:
            json.dump(rows, f, indent=1)


if __name__ == '__main__':
    main()
