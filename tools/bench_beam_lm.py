#!/usr/bin/env python3
"""Device CTC prefix beam search with an ARPA n-gram model (w2l_ctc_beam_search with lm) against the same search without one
(lm NULL): N=32 utterances, T in {500, 1000}, 29 labels, k in {5, 16, 32}, the posteriors of
tools/bench_beam.py.  The model is a synthetic suffix-closed 3-gram generated at run time (a vocabulary of random letter
strings; nothing is committed), loaded by ngram_lm.ArpaLM.  Also reported: the device table build (w2l_ngram_lm_build,
host-to-device copies included) and the host prefix_beam_search with the ArpaLM on one float64 utterance.

    python tools/bench_beam_lm.py [--vocab 20000] [--bigrams 400000] [--trigrams 600000] [--reps 5] [--host-k 5] [--json P]"""
import argparse
import ctypes as C
import functools
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_beam import peaky, time_launches  # noqa: E402
from wav2letter_pytorch_amd._lib import check, lib, ptr, stream_ptr  # noqa: E402
from wav2letter_pytorch_amd.beam_search import _label_info, prefix_beam_search, prefix_beam_search_gpu  # noqa: E402
from wav2letter_pytorch_amd.data.label_sets import english_labels  # noqa: E402
from wav2letter_pytorch_amd.ngram_lm import ArpaLM  # noqa: E402


def synthetic_arpa(path, vocab, n2, n3, seed=0):
    """a suffix-closed 3-gram: trigrams extend bigrams by an older word, bigrams extend unigrams"""
    rng = np.random.default_rng(seed)
    letters = np.array(list('ABCDEFGHIJKLMNOPQRSTUVWXYZ'))
    words = set()
    while len(words) < vocab:
        words.add(''.join(letters[rng.integers(0, 26, size=rng.integers(1, 8))]))
    words = sorted(words)
    tok = ['<unk>', '<s>', '</s>'] + words
    V = len(tok)
    big = set()
    while len(big) < n2:
        a = rng.integers(1, V, size=n2)                    # older word: <s> or a word
        b = rng.integers(2, V, size=n2)                    # newer word: </s> or a word
        big.update(zip(a[a != 2].tolist(), b[a != 2].tolist()))
    big = sorted(big)[:n2]
    bl = np.array(big)
    tri = set()
    while len(tri) < n3:
        pick = bl[rng.integers(0, len(bl), size=n3)]
        old = rng.integers(1, V, size=n3)
        keep = (old != 2) & (pick[:, 0] != 1)              # <s> only ever first
        tri.update(zip(old[keep].tolist(), pick[keep, 0].tolist(), pick[keep, 1].tolist()))
    tri = sorted(tri)[:n3]
    with open(path, 'w') as f:
        f.write('\\data\\\nngram 1=%d\nngram 2=%d\nngram 3=%d\n\n\\1-grams:\n' % (V, len(big), len(tri)))
        p1, b1 = -rng.uniform(1, 6, V), -rng.uniform(0, 1, V)
        p1[1] = -99
        f.write('\n'.join('%.5f\t%s\t%.5f' % (p1[i], tok[i], b1[i]) for i in range(V)))
        f.write('\n\n\\2-grams:\n')
        p2, b2 = -rng.uniform(0.2, 4, len(big)), -rng.uniform(0, 1, len(big))
        f.write('\n'.join('%.5f\t%s %s\t%.5f' % (p2[i], tok[a], tok[b], b2[i]) for i, (a, b) in enumerate(big)))
        f.write('\n\n\\3-grams:\n')
        p3 = -rng.uniform(0.1, 3, len(tri))
        f.write('\n'.join('%.5f\t%s %s %s' % (p3[i], tok[a], tok[b], tok[c]) for i, (a, b, c) in enumerate(tri)))
        f.write('\n\n\\end\\\n')


def time_lm_launches(x, k, reps, lm, tables, alpha=0.5, beta=5.0, prune=1e-3):
    n, t, a = x.shape
    info, end = _label_info(english_labels, 0, '>')
    info = info | np.array([ch.isspace() << 11 for ch in english_labels], dtype=np.int32)
    space = english_labels.index(' ')
    ws_bytes = int(lib.w2l_ctc_beam_search_workspace_bytes(n, t, k, lm.order))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=x.device)
    out = torch.empty(12 * n * k + 4 * n + 4 * n * k * t + 4 * n * k, dtype=torch.uint8, device=x.device)

    def launch():
        check(lib.w2l_ctc_beam_search(ptr(x), None, n, t, a, info.ctypes.data_as(C.c_void_p), 0, end, space, k, alpha, beta,
                                      prune, 0, tables.desc_ref, lm.order, None, 0, None, 0.0, ptr(ws), ws_bytes, ptr(out),
                                      stream_ptr()), 'w2l_ctc_beam_search')
    for _ in range(2):
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
    ap.add_argument('--vocab', type=int, default=20000)
    ap.add_argument('--bigrams', type=int, default=400000)
    ap.add_argument('--trigrams', type=int, default=600000)
    ap.add_argument('--alpha', type=float, default=0.5)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--host-k', default='5', help='beam widths at which the host decoder is timed at T=500 (empty: none)')
    ap.add_argument('--json', default=None)
    args = ap.parse_args()
    rows = []
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, 'synthetic.arpa')
        t0 = time.perf_counter()
        synthetic_arpa(path, args.vocab, args.bigrams, args.trigrams)
        t1 = time.perf_counter()
        lm = ArpaLM(path)
        t2 = time.perf_counter()
    lm.flat_tables()
    lm.spelling_trie(english_labels, 0)
    t3 = time.perf_counter()
    tables = lm.to_device(english_labels, 0, 'cuda')
    torch.cuda.synchronize()
    build = dict(what='tables', generate_s=round(t1 - t0, 2), parse_s=round(t2 - t1, 2), host_tables_s=round(t3 - t2, 2),
                 device_build_ms=round(tables.build_ms, 2), **lm.stats,
                 ngram_cap=tables.tables[0][2], trie_nodes=int(tables.trie_word.numel()), trie_cap=tables.tables[1][2])
    print(json.dumps(build), flush=True)
    rows.append(build)
    host_ks = {int(v) for v in args.host_k.split(',') if v}
    for t in (500, 1000):
        p = peaky(t, 32, t, len(english_labels))
        x = torch.from_numpy(p).cuda()
        for k in (5, 16, 32):
            ms0 = time_launches(x, k, args.reps)
            ms1 = time_lm_launches(x, k, args.reps, lm, tables, alpha=args.alpha)
            best0 = prefix_beam_search_gpu(x, english_labels, k=k)
            best1 = prefix_beam_search_gpu(x, english_labels, k=k, lm=lm, alpha=args.alpha)
            row = dict(N=32, T=t, A=len(english_labels), k=k, kernel_ms=round(ms0, 3), kernel_lm_ms=round(ms1, 3),
                       lm_overhead=round(ms1 / ms0 - 1, 3), changed_by_lm=sum(a != b for a, b in zip(best0, best1)))
            if t == 500 and k in host_ks:
                weigh = functools.lru_cache(maxsize=None)(lambda s: 10 ** lm.score(s))
                h0 = time.perf_counter()
                ref = prefix_beam_search(p[0].astype(np.float64), english_labels, lm=weigh, k=k, alpha=args.alpha)
                row['host_lm_one_utt_ms'] = round((time.perf_counter() - h0) * 1e3, 1)
                row['utt0_matches_host'] = ref == best1[0]
            rows.append(row)
            print(json.dumps(row), flush=True)
    if args.json:
        with open(args.json, 'w') as f:
            json.dump(rows, f, indent=1)


if __name__ == '__main__':
    main()
