#!/usr/bin/env python3
"""What the lexicon constraint costs the device CTC prefix beam searches: the four kernels {no LM, LM} x {no lexicon, lexicon}
(w2l_ctc_beam_search, _lex, _lm, _lm_lex) in one process on the posteriors of tools/bench_beam_lm.py: N=32 utterances, T in
{500, 1000}, 29 labels, k in {5, 16, 32}.  The model is that tool's synthetic 3-gram (a vocabulary of 20 000 random letter
strings plus <unk>, <s>, </s>); the lexicon is its vocabulary (Lexicon.from_lm), which shares the model's trie on the device.

Two sets of posteriors.  ``random``: that tool's (bursts of random characters): almost nothing they spell is a word of the
random vocabulary, so under the constraint the beam soon holds the few legal strings or empties, and the kernel stops at an
empty beam.  ``spelled``: the same look, but the bursts spell random words of the vocabulary with spaces between, so the
constrained search stays as busy as a real decode and the time difference is what the probes cost less what the smaller
candidate set saves.

Per (posteriors, T, k): kernel ms of each leg (events around ``reps`` launches after two warm-ups), the live candidates per
frame of each leg (the host recursion on utterance 0, whose candidates are the kernel's), and how many of the 32 decodes the
lexicon changed.

    python tools/bench_beam_lex.py [--vocab 20000] [--bigrams 400000] [--trigrams 600000] [--reps 5] [--live-t 500] [--json P]"""
import argparse
import ctypes as C
import functools
import json
import os
import sys
import tempfile

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_beam import peaky, time_launches  # noqa: E402
from bench_beam_lm import synthetic_arpa, time_lm_launches  # noqa: E402
from wav2letter_pytorch_amd._lib import check, lib, ptr, stream_ptr  # noqa: E402
from wav2letter_pytorch_amd.beam_search import _label_info, prefix_beam_search, prefix_beam_search_gpu  # noqa: E402
from wav2letter_pytorch_amd.data.label_sets import english_labels  # noqa: E402
from wav2letter_pytorch_amd.lexicon import Lexicon  # noqa: E402
from wav2letter_pytorch_amd.ngram_lm import ArpaLM  # noqa: E402


def time_lex_launches(x, k, reps, dev_lex, lm=None, tables=None, alpha=0.5, beta=5.0, prune=1e-3):
    """ms per launch of w2l_ctc_beam_search with the lexicon, and with ``lm`` if given"""
    n, t, a = x.shape
    info, end = _label_info(english_labels, 0, '>')
    info = info | np.array([ch.isspace() << 11 for ch in english_labels], dtype=np.int32)
    vp = info.ctypes.data_as(C.c_void_p)
    space = english_labels.index(' ')
    if lm is None:
        ws_bytes = int(lib.w2l_ctc_beam_search_workspace_bytes(n, t, k, 0))
    else:
        ws_bytes = int(lib.w2l_ctc_beam_search_workspace_bytes(n, t, k, lm.order))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=x.device)
    out = torch.empty(12 * n * k + 4 * n + 4 * n * k * t + 4 * n * k, dtype=torch.uint8, device=x.device)

    def launch():
        if lm is None:
            check(lib.w2l_ctc_beam_search(ptr(x), None, n, t, a, vp, 0, end, space, k, 0.0, beta, prune, 0, None, 0,
                                          dev_lex.desc_ref, 1, None, 0.0, ptr(ws), ws_bytes, ptr(out), stream_ptr()),
                  'w2l_ctc_beam_search')
        else:
            check(lib.w2l_ctc_beam_search(ptr(x), None, n, t, a, vp, 0, end, space, k, alpha, beta, prune, 0, tables.desc_ref,
                                          lm.order, dev_lex.desc_ref, 1, None, 0.0, ptr(ws), ws_bytes, ptr(out), stream_ptr()),
                  'w2l_ctc_beam_search')
    for _ in range(2):
        launch()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        launch()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps


def spelled(seed, n, t, words, labels, blank=0, boost=(6.0, 12.0), p_blank=0.6, max_burst=3):
    """bench_beam.peaky, but the bursts spell random ``words`` separated by spaces (a blank frame between equal neighbours)"""
    rng = np.random.default_rng(seed)
    a = len(labels)
    index = {ch: i for i, ch in enumerate(labels)}
    logits = rng.standard_normal((n, t, a))
    for u in range(n):
        text = ' '.join(words[i] for i in rng.integers(0, len(words), size=t // 4 + 1))
        f, pos, last = 0, 0, -1
        while f < t:
            c = index[text[pos]]
            if c == last or rng.random() < p_blank:
                logits[u, f, blank] += rng.uniform(*boost)
                f += 1
                last = -1
                continue
            burst = int(rng.integers(1, max_burst + 1))
            logits[u, f:f + burst, c] += rng.uniform(*boost)
            f += burst
            pos += 1
            last = c
    e = np.exp(logits - logits.max(-1, keepdims=True))
    return (e / e.sum(-1, keepdims=True)).astype(np.float32)


def live_per_frame(p, k, weigh, alpha, lexicon):
    """candidates with a positive mass per frame: the host recursion on one float64 utterance"""
    stats = {}
    prefix_beam_search(p.astype(np.float64), english_labels, lm=weigh, k=k, alpha=alpha, lexicon=lexicon, stats=stats)
    return round(stats['live'] / stats['frames'], 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--vocab', type=int, default=20000)
    ap.add_argument('--bigrams', type=int, default=400000)
    ap.add_argument('--trigrams', type=int, default=600000)
    ap.add_argument('--alpha', type=float, default=0.5)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--live-t', type=int, default=500, help='count live candidates on the host at this T only (0: never)')
    ap.add_argument('--json', default=None)
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, 'synthetic.arpa')
        synthetic_arpa(path, args.vocab, args.bigrams, args.trigrams)
        lm = ArpaLM(path)
    lex = Lexicon.from_lm(lm)
    tables = lm.to_device(english_labels, 0, 'cuda')
    dev_lex = lex.to_device(english_labels, 0, 'cuda')
    torch.cuda.synchronize()
    head = dict(what='lexicon', words=len(lex), vocab=lm.stats['vocab'], unspellable=lex.stats['unspellable'],
                trie_nodes=int(dev_lex.trie_word.numel()), trie_cap=int(dev_lex.trie_cap), shares_lm_trie=bool(dev_lex.shared))
    print(json.dumps(head), flush=True)
    rows = [head]
    weigh = functools.lru_cache(maxsize=None)(lambda s: 10 ** lm.score(s))
    for name, t in (('random', 500), ('random', 1000), ('spelled', 500), ('spelled', 1000)):
        if name == 'random':
            p = peaky(t, 32, t, len(english_labels))
        else:
            p = spelled(t, 32, t, lex.words, english_labels)
        x = torch.from_numpy(p).cuda()
        for k in (5, 16, 32):
            ms = dict(plain=time_launches(x, k, args.reps), lex=time_lex_launches(x, k, args.reps, dev_lex),
                      lm=time_lm_launches(x, k, args.reps, lm, tables, alpha=args.alpha),
                      lm_lex=time_lex_launches(x, k, args.reps, dev_lex, lm, tables, alpha=args.alpha))
            best = dict(plain=prefix_beam_search_gpu(x, english_labels, k=k),
                        lex=prefix_beam_search_gpu(x, english_labels, k=k, lexicon=lex),
                        lm=prefix_beam_search_gpu(x, english_labels, k=k, lm=lm, alpha=args.alpha),
                        lm_lex=prefix_beam_search_gpu(x, english_labels, k=k, lm=lm, alpha=args.alpha, lexicon='lm'))
            row = dict(posteriors=name, N=32, T=t, A=len(english_labels), k=k,
                       **{'ms_' + leg: round(v, 3) for leg, v in ms.items()},
                       lex_over_plain=round(ms['lex'] / ms['plain'] - 1, 3), lm_over_plain=round(ms['lm'] / ms['plain'] - 1, 3),
                       lm_lex_over_lm=round(ms['lm_lex'] / ms['lm'] - 1, 3),
                       changed_by_lexicon=sum(a != b for a, b in zip(best['plain'], best['lex'])),
                       changed_by_lexicon_lm=sum(a != b for a, b in zip(best['lm'], best['lm_lex'])),
                       empty_with_lexicon=sum(s == '' for s in best['lex']),
                       mean_len=round(float(np.mean([len(s) for s in best['plain']])), 1),
                       mean_len_lex=round(float(np.mean([len(s) for s in best['lex']])), 1),
                       # a result ends mid-word only where the final beam held no complete string; no other word leaves the list
                       results_mid_word=sum(not lex.complete(s) for s in best['lex']),
                       words_outside_lexicon=sum(w not in lex for leg in ('lex', 'lm_lex') for s in best[leg]
                                                 for w in (s.split() if lex.complete(s) else s.split()[:-1])))
            if t == args.live_t:
                for leg, (w, lx) in dict(plain=(None, None), lex=(None, lex), lm=(weigh, None), lm_lex=(weigh, lex)).items():
                    row['live_' + leg] = live_per_frame(p[0], k, w, args.alpha, lx)
            rows.append(row)
            print(json.dumps(row), flush=True)
    if args.json:
        with open(args.json, 'w') as f:
            json.dump(rows, f, indent=1)


if __name__ == '__main__':
    main()
