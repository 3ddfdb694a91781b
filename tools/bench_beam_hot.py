#!/usr/bin/env python3
"""What hotword boosting costs the device CTC prefix beam searches: each of the four kernels {no LM, LM} x {no lexicon, lexicon}
(w2l_ctc_beam_search with hotwords NULL) against its HOT instantiation (the same call with a hotword list) from the same build,
in one process, on the ``spelled`` posteriors of tools/bench_beam_lex.py (bursts that spell random words of the vocabulary): N=32
utterances, T in {500, 1000}, 29 labels, k in {5, 16, 32}.  The model, the lexicon and their shared trie are that tool's; the
hotwords are ``--hotwords`` words drawn from the vocabulary (so the posteriors do spell them), in a trie of their own.

Three legs per kernel: ``base`` (no hotwords), ``hot0`` (hotword_weight 0: the same search, candidate for candidate, so the
difference is the extra probe and the slot state alone) and ``hot`` (``--weight``: the boost changes which strings survive).
Timing: two warm-up launches per leg, then ``reps`` rounds that launch the three legs in turn, a device-event pair around every
launch; the median, min and max of each leg's ``reps`` times are reported.  Per (T, k) also: the live candidates per frame of the
base and hot legs (the host recursion on utterance 0, whose candidates are the kernel's), how many of the 32 decodes the boost
changed, and that every hot0 result (strings and weights) equals its base result.

    python tools/bench_beam_hot.py [--vocab 20000] [--bigrams 400000] [--trigrams 600000] [--hotwords 1000] [--weight 1.0]
                                   [--reps 5] [--live-t 500] [--json P]"""
import argparse
import ctypes as C
import functools
import json
import os
import statistics
import sys
import tempfile

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_beam_lex import spelled  # noqa: E402
from bench_beam_lm import synthetic_arpa  # noqa: E402
from wav2letter_pytorch_amd._lib import check, lib, ptr, stream_ptr  # noqa: E402
from wav2letter_pytorch_amd.beam_search import _label_info, prefix_beam_search, prefix_beam_search_gpu  # noqa: E402
from wav2letter_pytorch_amd.data.label_sets import english_labels  # noqa: E402
from wav2letter_pytorch_amd.lexicon import Lexicon  # noqa: E402
from wav2letter_pytorch_amd.ngram_lm import ArpaLM  # noqa: E402

COMBOS = ('plain', 'lex', 'lm', 'lm_lex')


def launcher(x, k, combo, lm, tables, dev_lex, dev_hot, weight, alpha, beta=5.0, prune=1e-3):
    """a callable that launches one search of ``combo`` on x: w2l_ctc_beam_search without hotwords (``dev_hot`` None) or with
    them at ``weight``.  Each launcher owns its workspace and output buffer."""
    n, t, a = x.shape
    info, end = _label_info(english_labels, 0, '>')
    info = info | np.array([ch.isspace() << 11 for ch in english_labels], dtype=np.int32)
    vp = info.ctypes.data_as(C.c_void_p)
    space = english_labels.index(' ')
    with_lm, with_lex = combo in ('lm', 'lm_lex'), combo in ('lex', 'lm_lex')
    ws_bytes = int(lib.w2l_ctc_beam_search_workspace_bytes(n, t, k, lm.order if with_lm else 0))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=x.device)
    out = torch.empty(12 * n * k + 4 * n + 4 * n * k * t + 4 * n * k, dtype=torch.uint8, device=x.device)
    head = (ptr(x), None, n, t, a, vp, 0, end)
    tail = (ptr(ws), ws_bytes, ptr(out), stream_ptr())
    lm_ref, order = (tables.desc_ref, lm.order) if with_lm else (None, 0)
    lex_ref = dev_lex.desc_ref if with_lex else None

    def launch():
        _keep = info                                   # (vp points into it)
        check(lib.w2l_ctc_beam_search(*head, space, k, alpha, beta, prune, 0, lm_ref, order, lex_ref, 1,
                                      dev_hot.desc_ref if dev_hot is not None else None, weight, *tail), 'w2l_ctc_beam_search')
    return launch


def time_in_turn(launches, reps, warmup=2):
    """ms of every launch: ``warmup`` launches of each leg, then ``reps`` rounds over the legs in turn, one device-event pair per
    launch.  Returns per leg (median, min, max)."""
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


def live_per_frame(p, k, weigh, alpha, lexicon, hot, weight):
    """candidates with a positive mass per frame: the host recursion on one float64 utterance"""
    stats = {}
    kw = dict(hotwords=hot, hotword_weight=weight) if hot is not None else {}
    prefix_beam_search(p.astype(np.float64), english_labels, lm=weigh, k=k, alpha=alpha, lexicon=lexicon, stats=stats, **kw)
    return round(stats['live'] / stats['frames'], 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--vocab', type=int, default=20000)
    ap.add_argument('--bigrams', type=int, default=400000)
    ap.add_argument('--trigrams', type=int, default=600000)
    ap.add_argument('--hotwords', type=int, default=1000)
    ap.add_argument('--weight', type=float, default=1.0)
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
    rng = np.random.default_rng(7)
    hot = Lexicon([lex.words[i] for i in sorted(rng.choice(len(lex.words), size=args.hotwords, replace=False))])
    tables = lm.to_device(english_labels, 0, 'cuda')
    dev_lex = lex.to_device(english_labels, 0, 'cuda')
    dev_hot = hot.to_device(english_labels, 0, 'cuda')
    torch.cuda.synchronize()
    head = dict(what='hotwords', hotwords=len(hot), weight=args.weight, hot_trie_nodes=int(dev_hot.trie_word.numel()),
                hot_trie_cap=int(dev_hot.trie_cap), vocab=lm.stats['vocab'], lexicon_trie_nodes=int(dev_lex.trie_word.numel()),
                reps=args.reps, device=torch.cuda.get_device_name(0))
    print(json.dumps(head), flush=True)
    rows = [head]
    weigh = functools.lru_cache(maxsize=None)(lambda s: 10 ** lm.score(s))
    for t in (500, 1000):
        p = spelled(t, 32, t, lex.words, english_labels)
        x = torch.from_numpy(p).cuda()
        for k in (5, 16, 32):
            row = dict(posteriors='spelled', N=32, T=t, A=len(english_labels), k=k)
            for combo in COMBOS:
                legs = dict(base=launcher(x, k, combo, lm, tables, dev_lex, None, 0.0, args.alpha),
                            hot0=launcher(x, k, combo, lm, tables, dev_lex, dev_hot, 0.0, args.alpha),
                            hot=launcher(x, k, combo, lm, tables, dev_lex, dev_hot, args.weight, args.alpha))
                ms = time_in_turn(legs, args.reps)
                for leg, (med, lo, hi) in ms.items():
                    row['ms_%s_%s' % (combo, leg)] = [round(med, 3), round(lo, 3), round(hi, 3)]
                row['%s_hot0_over_base' % combo] = round(ms['hot0'][0] / ms['base'][0] - 1, 3)
                row['%s_hot_over_base' % combo] = round(ms['hot'][0] / ms['base'][0] - 1, 3)
                kw = dict(k=k, return_weights=True)
                if combo in ('lm', 'lm_lex'):
                    kw.update(lm=lm, alpha=args.alpha)
                if combo in ('lex', 'lm_lex'):
                    kw.update(lexicon='lm' if combo == 'lm_lex' else lex)
                base = prefix_beam_search_gpu(x, english_labels, **kw)
                zero = prefix_beam_search_gpu(x, english_labels, hotwords=hot, hotword_weight=0.0, **kw)
                boosted = prefix_beam_search_gpu(x, english_labels, hotwords=hot, hotword_weight=args.weight, **kw)
                row['%s_hot0_equals_base' % combo] = zero == base
                row['%s_changed_by_hot' % combo] = sum(a[0] != b[0] for a, b in zip(base, boosted))
                row['%s_hot_chars' % combo] = [int(np.sum([hot.boost_chars(s) for s, _ in res])) for res in (base, boosted)]
                if t == args.live_t:
                    w, lx = (weigh if combo in ('lm', 'lm_lex') else None), (lex if combo in ('lex', 'lm_lex') else None)
                    row['live_%s' % combo] = [live_per_frame(p[0], k, w, args.alpha, lx, None, 0.0),
                                              live_per_frame(p[0], k, w, args.alpha, lx, hot, args.weight)]
            rows.append(row)
            print(json.dumps(row), flush=True)
            if args.json:
                with open(args.json, 'w') as f:
                    json.dump(rows, f, indent=1)


if __name__ == '__main__':
    main()
