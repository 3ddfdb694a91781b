#!/usr/bin/env python3
"""What a lexicon and hotwords cost the device ASG beam search: the eight instantiations of asg_beam_search_kernel<LM, LEX, HOT>
(w2l_asg_beam_search_tables with each table NULL or given) in one process, interleaved, at the shapes and on the inputs of
tools/bench_asg_beam.py: N=32 utterances, T=500 frames, 29 labels, k in {5, 32}, the held scores, the random transitions and
the generated trigram model of that tool.  The lexicon is the model's vocabulary (the words of one to three letters of ABCDE,
its trie shared with the model's on the device); the hotwords are ``--hotwords`` words drawn from it, in a trie of their own.

Timing: two warm-up launches per leg, then ``--reps`` rounds that launch the legs in turn, a device-event pair around every
launch; the median, min and max of each leg's times are reported, and each instantiation against ``<LM,0,0>`` of the same
run.  ``old`` is w2l_asg_beam_search, the symbol without the two word lists, as one more leg per LM setting: it launches
``<LM,0,0>`` too, so old / <LM,0,0> is the launch-to-launch spread of this bench.  With ``--parent-lib`` (the library of the
commit before the word lists) its w2l_asg_beam_search is timed in the same rounds as ``parent``.  Per k also: how many of the
32 decodes the lexicon and the hotwords change, and that weight 0 gives the strings and weights of no hotwords.

    python tools/bench_asg_beam_lex.py [--reps 7] [--hotwords 20] [--weight 1.0] [--parent-lib PATH] [--json PATH]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import tempfile

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_asg_beam import held_scores, write_arpa  # noqa: E402
from wav2letter_pytorch_amd import asg_beam  # noqa: E402
from wav2letter_pytorch_amd._lib import _SIGNATURES, check, lib, ptr, stream_ptr  # noqa: E402
from wav2letter_pytorch_amd.data.label_sets import english_labels  # noqa: E402
from wav2letter_pytorch_amd.lexicon import Lexicon  # noqa: E402
from wav2letter_pytorch_amd.ngram_lm import ArpaLM  # noqa: E402

VP = C.c_void_p
COMBOS = [(lm, lex, hot) for lm in (0, 1) for lex in (0, 1) for hot in (0, 1)]


def leg_name(combo):
    return '<%d,%d,%d>' % combo


def launcher(x, g, k, combo, lm, tables, dev_lex, dev_hot, weight, alpha, old_from=None, beta=5.0, prune=1e-3):
    """a callable that launches one search on x: w2l_asg_beam_search_tables with the tables of ``combo``, or (``old_from``: a
    loaded library) that library's w2l_asg_beam_search.  Each launcher owns its workspace and output buffer."""
    n, t, a = x.shape
    with_lm, with_lex, with_hot = combo
    info = asg_beam._label_info(english_labels, True)
    space = english_labels.index(' ')
    order = lm.order if with_lm else 0
    ws_bytes = int(lib.w2l_asg_beam_search_workspace_bytes(n, t, a, k, order))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=x.device)
    out = torch.empty(12 * n * k + 4 * n + 4 * n * k * t + 4 * n * k, dtype=torch.uint8, device=x.device)
    head = (ptr(x), ptr(g), None, n, t, a, info.ctypes.data_as(VP), 0, space, k, alpha, beta, prune,
            tables.desc_ref if with_lm else None, order)
    tail = (ptr(ws), ws_bytes, ptr(out), stream_ptr())
    words = (dev_lex.desc_ref if with_lex else None, 1, dev_hot.desc_ref if with_hot else None, weight)

    def launch():
        _keep = info                                   # (head points into it)
        if old_from is not None:
            rc = old_from.w2l_asg_beam_search(*head, *tail)
            if rc:
                raise RuntimeError('w2l_asg_beam_search of the other library failed (code %d)' % rc)
        else:
            check(lib.w2l_asg_beam_search_tables(*head, *words, *tail), 'w2l_asg_beam_search_tables')
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


def load_other(path):
    """another build of the library, for its w2l_asg_beam_search alone"""
    other = C.CDLL(path)
    res, args = _SIGNATURES['w2l_asg_beam_search']
    other.w2l_asg_beam_search.restype = res
    other.w2l_asg_beam_search.argtypes = args
    return other


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--hotwords', type=int, default=20)
    ap.add_argument('--weight', type=float, default=1.0)
    ap.add_argument('--alpha', type=float, default=0.5)
    ap.add_argument('--parent-lib', default=None)
    ap.add_argument('--json', default=None)
    args = ap.parse_args()
    n, t, a = 32, 500, len(english_labels)
    x = torch.from_numpy(held_scores(7, n, t, english_labels)).cuda()
    g = torch.from_numpy((0.5 * np.random.default_rng(8).standard_normal((a, a))).astype(np.float32)).cuda()
    with tempfile.TemporaryDirectory() as d:
        write_arpa(os.path.join(d, 'bench.arpa'))
        lm = ArpaLM(os.path.join(d, 'bench.arpa'))
    lex = Lexicon.from_lm(lm)
    rng = np.random.default_rng(7)
    hot = Lexicon([lex.words[i] for i in sorted(rng.choice(len(lex.words), size=args.hotwords, replace=False))])
    tables = lm.to_device(english_labels, 0, 'cuda')
    dev_lex = lex.to_device(english_labels, 0, 'cuda')
    dev_hot = hot.to_device(english_labels, 0, 'cuda')
    parent = load_other(args.parent_lib) if args.parent_lib else None
    torch.cuda.synchronize()
    head = dict(what='asg lexicon / hotwords', N=n, T=t, A=a, lexicon_words=len(lex), lexicon_shares_lm_trie=bool(dev_lex.shared),
                hotwords=len(hot), weight=args.weight, alpha=args.alpha, reps=args.reps, parent_lib=bool(parent),
                device=torch.cuda.get_device_name(0))
    print(json.dumps(head), flush=True)
    rows = [head]
    for k in (5, 32):
        mk = lambda combo, **kw: launcher(x, g, k, combo, lm, tables, dev_lex, dev_hot, args.weight, args.alpha, **kw)  # noqa: E731
        legs = {}
        for with_lm in (0, 1):
            if parent is not None:
                legs['parent<%d>' % with_lm] = mk((with_lm, 0, 0), old_from=parent)
            legs['old<%d>' % with_lm] = mk((with_lm, 0, 0), old_from=lib)
            for combo in COMBOS:
                if combo[0] == with_lm:
                    legs[leg_name(combo)] = mk(combo)
        ms = time_in_turn(legs, args.reps)
        row = dict(k=k)
        for leg, (med, lo, hi) in ms.items():
            row['ms_' + leg] = [round(med, 3), round(lo, 3), round(hi, 3)]
        for combo in COMBOS:
            base = ms[leg_name((combo[0], 0, 0))][0]
            if combo[1:] != (0, 0):
                row[leg_name(combo) + '_over_base'] = round(ms[leg_name(combo)][0] / base - 1, 3)
        for with_lm in (0, 1):
            base = ms[leg_name((with_lm, 0, 0))][0]
            row['old<%d>_over_base' % with_lm] = round(ms['old<%d>' % with_lm][0] / base - 1, 3)
            if parent is not None:
                row['base_over_parent<%d>' % with_lm] = round(base / ms['parent<%d>' % with_lm][0] - 1, 3)
        # the strings of the timed searches, for the record
        for with_lm in (0, 1):
            kw = dict(k=k, return_weights=True)
            if with_lm:
                kw.update(lm=lm, alpha=args.alpha)
            plain = asg_beam.asg_beam_search_gpu(x, g, english_labels, **kw)
            lexed = asg_beam.asg_beam_search_gpu(x, g, english_labels, lexicon=lex, **kw)
            zero = asg_beam.asg_beam_search_gpu(x, g, english_labels, hotwords=hot, hotword_weight=0.0, **kw)
            boosted = asg_beam.asg_beam_search_gpu(x, g, english_labels, hotwords=hot, hotword_weight=args.weight, **kw)
            tag = 'lm' if with_lm else 'plain'
            row[tag + '_changed_by_lexicon'] = sum(u[0] != v[0] for u, v in zip(plain, lexed))
            row[tag + '_changed_by_hotwords'] = sum(u[0] != v[0] for u, v in zip(plain, boosted))
            row[tag + '_hot0_equals_base'] = zero == plain
            row[tag + '_all_words_in_lexicon'] = all(w in lex for s, _ in lexed for w in s.split())
        rows.append(row)
        print(json.dumps(row), flush=True)
        if args.json:
            with open(args.json, 'w') as f:
                json.dump(rows, f, indent=1)


if __name__ == '__main__':
    main()
