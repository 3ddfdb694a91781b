"""Cases shared by the word-list tests of the ASG beam search (test_cpu_asg_lexicon.py, test_gpu_asg_lexicon.py): a brute-force
reference for the lexicon-constrained masses (it enumerates frame paths: tiny shapes only) and the constructed frame sequence
on which the participation rule without its lexicon amendment empties the beam."""
import itertools
import math

import numpy as np

from asg_beam_refs import logsumexp, path_score, text_of
from wav2letter_pytorch_amd.asg import collapse_frames

LABELS4 = ['_', ' ', 'A', 'L']                                  # the repeat label, the space, two letters


def brute_constrained_masses(x, g, labels, lexicon, repeat=0):
    """dict encoded hypothesis -> log-sum of the scores of the frame paths that read it and whose every prefix (the path's
    first 1, 2, ... frames) reads a legal text"""
    t_n, a = x.shape
    per_hyp = {}
    for path in itertools.product(range(a), repeat=t_n):
        prefixes = [tuple(collapse_frames(path[:t + 1])[0]) for t in range(t_n)]
        if all(lexicon.allows(text_of(e, labels, repeat), end_char='') for e in prefixes):
            per_hyp.setdefault(prefixes[-1], []).append(path_score(x, g, path))
    return {e: logsumexp(v) for e, v in per_hyp.items()}


# ---- the participation-rule case.  Lexicon {'AL'}, k = 1, prune = 1e-3.  Frame 0 makes ('A',) the only member.  In frame 1
# only the space passes the prune (it is the argmax too), 'A ' is illegal ('A' is no word) and the member's last label A does
# not pass: by "x > log(prune) or the argmax" alone nothing gets mass and the beam is empty.  With the amendment A takes part
# as the last label of a member, the member stays, and frame 2 spells 'AL'.
DEAD_LABELS = LABELS4
DEAD_WORDS = ['AL']
DEAD_K, DEAD_PRUNE = 1, 1e-3


def dead_beam_case():
    """-> (x float32 [3, 4], g float32 [4, 4])"""
    x = np.full((3, 4), -9.0, dtype=np.float32)
    x[0, 2] = -0.01                                             # A
    x[1, 1] = -0.001                                            # the space
    x[2, 3] = -0.01                                             # L
    g = (0.1 * np.random.default_rng(5).standard_normal((4, 4))).astype(np.float32)
    return x, g


def unamended_participants(frame, prune):
    """the labels of a frame by the rule without a lexicon: above the prune, or the first argmax"""
    first = int(np.argmax(frame))
    return [c for c in range(len(frame)) if prune <= 0 or frame[c] > math.log(prune) or c == first]


def write_arpa(path, words, order, seed, per_order=60):
    """a random order-``order`` ARPA model over ``words``: every higher n-gram extends a lower one by an older word"""
    from wav2letter_pytorch_amd.ngram_lm import ArpaLM
    rng = np.random.default_rng(seed)
    lines = {1: ['-2.0\t<unk>', '-99\t<s>\t%.5f' % -rng.uniform(0, 0.5), '%.5f\t</s>' % -rng.uniform(0.3, 1.5)]}
    lines[1] += ['%.5f\t%s\t%.5f' % (-rng.uniform(0.3, 2.5), w, -rng.uniform(0, 0.6)) for w in words]
    grams = [(w,) for w in words + ['</s>']]
    for n in range(2, order + 1):
        cur = set()
        while len(cur) < per_order:
            base = grams[rng.integers(len(grams))]
            if base[0] != '<s>':
                cur.add(((['<s>'] + words)[rng.integers(len(words) + 1)],) + base)
        grams = sorted(cur)
        lines[n] = ['%.5f\t%s' % (-rng.uniform(0.05, 1.5), ' '.join(gr)) + ('' if n == order else '\t%.5f' % -rng.uniform(0, 0.6))
                    for gr in grams]
    text = '\\data\\\n' + ''.join('ngram %d=%d\n' % (n, len(lines[n])) for n in lines)
    for n in lines:
        text += '\n\\%d-grams:\n' % n + '\n'.join(lines[n]) + '\n'
    path.write_text(text + '\n\\end\\\n')
    return ArpaLM(str(path))
