#!/usr/bin/env python3
"""What minimum-Bayes-risk selection costs behind a device beam search, and what the device edit distance saves: N=32
utterances, T=500, 29 labels, k in {5, 32, 64}, word and char unit, on the ``spelled`` posteriors of tools/bench_beam_lex.py
(bursts that spell random words, so the n-best rows are sentences that differ in a few words).

Three figures per (k, unit):
  (a) ``mbr``     the launches of w2l_nbest_mbr (tokenise, distances, risk) on the search's out buffer
  (b) ``search``  the w2l_ctc_beam_search launch of the same shape that MBR follows
  (c) ``host``    w2l_levenshtein_host over the same pairs of token sequences, one call a pair, on one host thread (the
                  tokenising is outside the clock; wall time, ``--host-reps`` runs, the fastest)
(a) and (b) from the same process: two warm-up launches each, then ``reps`` rounds that launch the two in turn with a
device-event pair around every launch; median, min and max of the ``reps`` times.  Also per row: the pairs, the mean tokens per
row, and how many of the 32 picks are not rank 0.

    python tools/bench_mbr.py [--reps 7] [--host-reps 2] [--json P]"""
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_beam_lex import spelled  # noqa: E402
from wav2letter_pytorch_amd import mbr  # noqa: E402
from wav2letter_pytorch_amd._lib import check, lib, ptr, stream_ptr  # noqa: E402
from wav2letter_pytorch_amd.beam_search import _label_info, search_out_layout, split_search_out  # noqa: E402
from wav2letter_pytorch_amd.data.label_sets import english_labels  # noqa: E402

N, T = 32, 500


def vocabulary(size=2000, seed=3):
    rng = np.random.default_rng(seed)
    letters = english_labels[2:28]
    return sorted({''.join(letters[i] for i in rng.integers(0, 26, size=int(rng.integers(1, 9)))) for _ in range(size)})


def launchers(x, k, unit):
    """(search, mbr): callables that launch w2l_ctc_beam_search on x and w2l_nbest_mbr on its results; plus the buffer"""
    n, t, a = x.shape
    info, end = _label_info(english_labels, 0, '>')
    vp = info.ctypes.data_as(C.c_void_p)
    ws_bytes = int(lib.w2l_ctc_beam_search_workspace_bytes(n, t, k, 0))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=x.device)
    lay = search_out_layout(n, k, t, False)
    at = mbr.mbr_offset(lay.beam_bytes)
    out = torch.empty(at + mbr.mbr_sections(n, k, t).total, dtype=torch.uint8, device=x.device)
    cls = mbr.label_classes(english_labels)
    mws_bytes = int(lib.w2l_nbest_mbr_workspace_bytes(n, k, t))
    mws = torch.empty(mws_bytes, dtype=torch.uint8, device=x.device)

    def search():
        _keep = info
        check(lib.w2l_ctc_beam_search(ptr(x), None, n, t, a, vp, 0, end, -1, k, 0.3, 5.0, 1e-3, 0, None, 0, None, 1, None, 0.0,
                                      ptr(ws), ws_bytes, ptr(out), stream_ptr()), 'w2l_ctc_beam_search')

    def select():
        check(lib.w2l_nbest_mbr(ptr(out), n, k, t, cls.ctypes.data_as(C.c_void_p), len(cls), mbr.UNITS.index(unit), -1, 1.0,
                                ptr(mws), mws_bytes, C.c_void_p(out.data_ptr() + at), stream_ptr()), 'w2l_nbest_mbr')

    return search, select, out, at


def time_in_turn(launches, reps, warmup=2):
    for launch in launches.values():
        for _ in range(warmup):
            launch()
    torch.cuda.synchronize()
    pairs = {leg: [] for leg in launches}
    for _ in range(reps):
        for leg, launch in launches.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            launch()
            e.record()
            pairs[leg].append((s, e))
    torch.cuda.synchronize()
    ms = {leg: [s.elapsed_time(e) for s, e in v] for leg, v in pairs.items()}
    return {leg: (statistics.median(v), min(v), max(v)) for leg, v in ms.items()}


def host_pairs(lengths, idx, unit):
    """the token sequences of every present row and the (i, j) pairs MBR scores, as int32 arrays for w2l_levenshtein_host"""
    vocab = {}
    jobs = []
    tokens = 0
    rows = 0
    for u in range(lengths.shape[0]):
        seqs = []
        for r in range(lengths.shape[1]):
            if lengths[u, r] < 0:
                continue
            text = ''.join(english_labels[j] for j in idx[u, r, :lengths[u, r]])
            if unit == 'word':
                seq = np.array([vocab.setdefault(w, len(vocab)) for w in mbr.words_of(text)], dtype=np.int32)
            else:
                seq = np.array([ord(c) for c in mbr.chars_of(text)], dtype=np.int32)
            seqs.append(seq)
            tokens += len(seq)
            rows += 1
        jobs += [(seqs[i], seqs[j]) for i in range(len(seqs)) for j in range(i + 1, len(seqs))]
    return jobs, tokens / max(rows, 1)


def host_ms(jobs, reps):
    vp = C.c_void_p
    args = [(a.ctypes.data_as(vp), len(a), b.ctypes.data_as(vp), len(b)) for a, b in jobs]
    best = float('inf')
    for _ in range(reps):
        t0 = time.perf_counter()
        for arg in args:
            lib.w2l_levenshtein_host(*arg)
        best = min(best, (time.perf_counter() - t0) * 1e3)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--host-reps', type=int, default=2)
    ap.add_argument('--json', default=None)
    args = ap.parse_args()
    x = torch.from_numpy(spelled(11, N, T, vocabulary(), english_labels)).cuda()
    head = dict(what='mbr', N=N, T=T, A=len(english_labels), reps=args.reps, device=torch.cuda.get_device_name(0))
    print(json.dumps(head), flush=True)
    rows = [head]
    for k in (5, 32, 64):
        for unit in mbr.UNITS:
            search, select, out, at = launchers(x, k, unit)
            ms = time_in_turn(dict(search=search, mbr=select), args.reps)
            host = out.cpu().numpy()
            _, lengths, _, idx, _ = split_search_out(host, N, k, T, False)
            res = mbr.split_mbr(host[at:], N, k, T)
            jobs, mean_tokens = host_pairs(lengths, idx, unit)
            h = host_ms(jobs, args.host_reps)
            row = dict(k=k, unit=unit, pairs=len(jobs), mean_tokens=round(mean_tokens, 1),
                       ms_mbr=[round(v, 3) for v in ms['mbr']], ms_search=[round(v, 3) for v in ms['search']],
                       ms_host=round(h, 1), mbr_over_search=round(ms['mbr'][0] / ms['search'][0], 4),
                       host_over_mbr=round(h / ms['mbr'][0], 1), status=int(res.status.sum()),
                       picks_not_rank0=int((res.pick != 0).sum()))
            rows.append(row)
            print(json.dumps(row), flush=True)
            if args.json:
                with open(args.json, 'w') as f:
                    json.dump(rows, f, indent=1)


if __name__ == '__main__':
    main()
