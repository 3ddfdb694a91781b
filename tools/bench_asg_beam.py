#!/usr/bin/env python3
"""ASG decoding launches against their CTC counterparts at the same shape, in one process, alternating: N=32 utterances, T'=500
output frames, 29 labels, k in {5, 32}.

    w2l_asg_beam_search      against  w2l_ctc_beam_search
    the same two with lm     (a generated trigram model over short words)
    w2l_asg_align            against  w2l_ctc_align            (targets of 80 labels)

Both searches read the SAME log-probabilities: labels held for a few frames each, a rival almost as likely, a trained ASG
model's look (index 0 is the repeat label for the one and the blank for the other, a label like any other here).  Times are
CUDA events around back-to-back launches after warm-up (kernel only); every pair is measured in ``--rounds`` alternating
windows and the median window is reported with the spread (min .. max).

    python tools/bench_asg_beam.py [--reps 10] [--rounds 5] [--json PATH]"""
import argparse
import ctypes as C
import itertools
import json
import os
import sys
import tempfile

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from wav2letter_pytorch_amd import asg_beam  # noqa: E402
from wav2letter_pytorch_amd._lib import check, lib, ptr, stream_ptr  # noqa: E402
from wav2letter_pytorch_amd.alignment import align_sections  # noqa: E402
from wav2letter_pytorch_amd.beam_search import _label_info  # noqa: E402
from wav2letter_pytorch_amd.data.label_sets import english_labels  # noqa: E402
from wav2letter_pytorch_amd.ngram_lm import ArpaLM  # noqa: E402

VP = C.c_void_p
LETTERS = 'ABCDE'


def held_scores(seed, n, t, labels, p_space=0.25, boost=(4.0, 9.0), rival=2.0):
    """float32 log-softmax [n, t, labels]: every label held for 2 to 6 frames, a rival label boosted almost as much"""
    rng = np.random.default_rng(seed)
    a = len(labels)
    cand = [labels.index(c) for c in LETTERS]
    space = labels.index(' ')
    logits = rng.standard_normal((n, t, a))
    for u in range(n):
        f = 0
        while f < t:
            c = space if rng.random() < p_space else (0 if rng.random() < 0.15 else cand[rng.integers(len(cand))])
            burst = int(rng.integers(2, 7))
            b = rng.uniform(*boost)
            logits[u, f:f + burst, c] += b
            logits[u, f:f + burst, cand[rng.integers(len(cand))]] += b - rng.uniform(0, rival)
            f += burst
    z = logits - logits.max(-1, keepdims=True)
    return (z - np.log(np.exp(z).sum(-1, keepdims=True))).astype(np.float32)


def write_arpa(path, seed=1, per_order=2000):
    """a trigram model over the words of one to three LETTERS"""
    rng = np.random.default_rng(seed)
    words = [''.join(w) for n in (1, 2, 3) for w in itertools.product(LETTERS, repeat=n)]
    lines = {1: ['-2.0\t<unk>', '-99\t<s>\t-0.3', '-1.0\t</s>\t0']}
    lines[1] += ['%.5f\t%s\t%.5f' % (-rng.uniform(0.3, 2.5), w, -rng.uniform(0, 0.6)) for w in words]
    grams = [(w,) for w in words + ['</s>']]
    for n in (2, 3):
        cur = set()
        while len(cur) < per_order:
            base = grams[rng.integers(len(grams))]
            if base[0] != '<s>':
                cur.add(((['<s>'] + words)[rng.integers(len(words) + 1)],) + base)
        grams = sorted(cur)
        lines[n] = ['%.5f\t%s' % (-rng.uniform(0.05, 1.5), ' '.join(g)) + ('' if n == 3 else '\t%.5f' % -rng.uniform(0, 0.6))
                    for g in grams]
    text = '\\data\\\n' + ''.join('ngram %d=%d\n' % (n, len(lines[n])) for n in lines)
    for n in lines:
        text += '\n\\%d-grams:\n' % n + '\n'.join(lines[n]) + '\n'
    with open(path, 'w') as f:
        f.write(text + '\n\\end\\\n')


def window(launch, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        launch()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps


def alternate(a, b, reps, rounds):
    """-> ((median, min, max) of a, the same of b), ms per launch, windows alternating a, b, a, b, ..."""
    for _ in range(3):
        a()
        b()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(rounds):
        ta.append(window(a, reps))
        tb.append(window(b, reps))
    stat = lambda v: (round(float(np.median(v)), 3), round(min(v), 3), round(max(v), 3))      # noqa: E731
    return stat(ta), stat(tb)


def search_pair(x, g, k, lm, beta=5.0, prune=1e-3, alpha=0.5):
    n, t, a = x.shape
    dev = x.device
    labels = english_labels
    ctc_info, end = _label_info(labels, 0, '>')
    asg_info = asg_beam._label_info(labels, lm is not None)
    space = labels.index(' ')
    extra = 4 * n * k if lm is not None else 0
    out_a = torch.empty(12 * n * k + 4 * n + 4 * n * k * t + extra, dtype=torch.uint8, device=dev)
    out_c = torch.empty_like(out_a)
    tables, lm_ref, order = None, None, 0
    if lm is not None:
        ctc_info = ctc_info | np.array([ch.isspace() << 11 for ch in labels], dtype=np.int32)
        tables = lm.to_device(labels, 0, dev)
        lm_ref, order = tables.desc_ref, lm.order
    wa = int(lib.w2l_asg_beam_search_workspace_bytes(n, t, a, k, order))
    wc = int(lib.w2l_ctc_beam_search_workspace_bytes(n, t, k, order))
    ws_a = torch.empty(wa, dtype=torch.uint8, device=dev)
    ws_c = torch.empty(wc, dtype=torch.uint8, device=dev)

    def asg():
        _keep = tables                                 # (lm_ref points at its device tables)
        check(lib.w2l_asg_beam_search(ptr(x), ptr(g), None, n, t, a, asg_info.ctypes.data_as(VP), 0, space, k, alpha, beta, prune,
                                      lm_ref, order, ptr(ws_a), wa, ptr(out_a), stream_ptr()), 'w2l_asg_beam_search')

    def ctc():
        check(lib.w2l_ctc_beam_search(ptr(x), None, n, t, a, ctc_info.ctypes.data_as(VP), 0, end, space, k, alpha, beta, prune, 1,
                                      lm_ref, order, None, 0, None, 0.0, ptr(ws_c), wc, ptr(out_c), stream_ptr()),
              'w2l_ctc_beam_search')
    return asg, ctc


def align_pair(x, g, smax, seed=3):
    n, t, a = x.shape
    dev = x.device
    rng = np.random.default_rng(seed)
    tg = rng.integers(1, a, size=(n, smax)).astype(np.int32)
    tl = np.full(n, smax, dtype=np.int32)
    tgt = torch.from_numpy(np.concatenate([tg.reshape(-1), tl])).to(dev)
    o = align_sections(n, t, smax)
    out_a = torch.empty(o[5], dtype=torch.uint8, device=dev)
    out_c = torch.empty(o[5], dtype=torch.uint8, device=dev)
    wa = int(lib.w2l_asg_align_workspace_bytes(n, t, a, smax))
    wc = int(lib.w2l_ctc_align_workspace_bytes(n, t, smax))
    ws_a = torch.empty(max(wa, 4), dtype=torch.uint8, device=dev)
    ws_c = torch.empty(max(wc, 4), dtype=torch.uint8, device=dev)
    tp, lp = tgt.data_ptr(), tgt.data_ptr() + 4 * n * smax
    sect = lambda out: [VP(out.data_ptr() + o[i]) for i in range(5)]      # noqa: E731
    sa, sc = sect(out_a), sect(out_c)

    def asg():
        check(lib.w2l_asg_align(ptr(x), ptr(g), None, VP(tp), smax, VP(lp), 1, n, t, a, smax, 0, 0, ptr(ws_a), wa, *sa,
                                stream_ptr()), 'w2l_asg_align')

    def ctc():
        check(lib.w2l_ctc_align(ptr(x), None, VP(tp), smax, VP(lp), 1, n, t, a, smax, 0, 1, ptr(ws_c), wc, *sc, stream_ptr()),
              'w2l_ctc_align')
    return asg, ctc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--json', default=None)
    args = ap.parse_args()
    n, t, a = 32, 500, len(english_labels)
    p = held_scores(7, n, t, english_labels)
    x = torch.from_numpy(p).cuda()
    g = torch.from_numpy((0.5 * np.random.default_rng(8).standard_normal((a, a))).astype(np.float32)).cuda()
    passing = round(float((p > np.log(1e-3)).sum(-1).mean()), 2)
    with tempfile.TemporaryDirectory() as d:
        write_arpa(os.path.join(d, 'bench.arpa'))
        lm = ArpaLM(os.path.join(d, 'bench.arpa'))
    rows = []
    for name, use_lm in (('beam_search', False), ('beam_search_lm', True)):
        for k in (5, 32):
            asg, ctc = search_pair(x, g, k, lm if use_lm else None)
            ta, tc = alternate(asg, ctc, args.reps, args.rounds)
            rows.append(dict(launch=name, N=n, T=t, A=a, k=k, labels_per_frame=passing, asg_ms=ta[0], asg_min_max=ta[1:],
                             ctc_ms=tc[0], ctc_min_max=tc[1:], asg_over_ctc=round(ta[0] / tc[0], 3)))
            print(json.dumps(rows[-1]), flush=True)
    asg, ctc = align_pair(x, g, 80)
    ta, tc = alternate(asg, ctc, args.reps * 10, args.rounds)
    rows.append(dict(launch='align', N=n, T=t, A=a, S=80, asg_ms=ta[0], asg_min_max=ta[1:], ctc_ms=tc[0], ctc_min_max=tc[1:],
                     asg_over_ctc=round(ta[0] / tc[0], 3)))
    print(json.dumps(rows[-1]), flush=True)
    # the strings of the timed search, for the record: how long they are and how often the LM changes them
    plain = asg_beam.asg_beam_search_gpu(x, g, english_labels, k=32)
    with_lm = asg_beam.asg_beam_search_gpu(x, g, english_labels, k=32, lm=lm, alpha=0.5)
    rows.append(dict(mean_len=round(float(np.mean([len(s) for s in plain])), 1),
                     lm_changes=sum(u != v for u, v in zip(plain, with_lm))))
    print(json.dumps(rows[-1]), flush=True)
    if args.json:
        with open(args.json, 'w') as f:
            json.dump(rows, f, indent=1)


if __name__ == '__main__':
    main()
