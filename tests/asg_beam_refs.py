"""Brute-force references and input generators shared by the ASG beam-search / alignment tests (test_cpu_asg_beam.py,
test_gpu_asg_beam.py, test_gpu_asg_align.py).  Everything here enumerates frame paths, so it is for tiny shapes only."""
import itertools

import numpy as np

from wav2letter_pytorch_amd.asg import collapse_frames, decode_repeats

SMALL_LABELS = ['_', 'a', 'b']


def small_case(seed, a=3, t=4):
    """the issue's exhaustive case: x ~ 2 N(0, 1), g ~ N(0, 1), float64"""
    rng = np.random.default_rng(seed)
    return 2.0 * rng.standard_normal((t, a)), rng.standard_normal((a, a))


def path_score(x, g, path):
    s = x[0, path[0]]
    for t in range(1, len(path)):
        s = s + g[path[t - 1], path[t]] + x[t, path[t]]
    return float(s)


def logsumexp(values):
    v = np.asarray(values, dtype=np.float64)
    m = v.max()
    return float(m + np.log(np.exp(v - m).sum()))


def brute_masses(x, g):
    """-> (dict encoded hypothesis -> log-sum of its frame paths' scores, Z_full, the best frame path)"""
    t_n, a = x.shape
    per_hyp, scores, best = {}, [], None
    for path in itertools.product(range(a), repeat=t_n):
        s = path_score(x, g, path)
        scores.append(s)
        per_hyp.setdefault(tuple(collapse_frames(path)[0]), []).append(s)
        if best is None or s > best[0]:
            best = (s, path)
    return {e: logsumexp(v) for e, v in per_hyp.items()}, logsumexp(scores), best[1]


def text_of(encoded, labels, repeat=0):
    return ''.join(labels[i] for i in decode_repeats(encoded, repeat))


def brute_align(x, g, encoded):
    """the best score over the frame paths that read ``encoded`` (None if there is none)"""
    t_n, a = x.shape
    best = None
    for path in itertools.product(range(a), repeat=t_n):
        if collapse_frames(path)[0] == list(encoded):
            s = path_score(x, g, path)
            if best is None or s > best:
                best = s
    return best


def log_softmax_scores(seed, shape, scale=1.0):
    """float32 log-softmax of seeded normals"""
    rng = np.random.default_rng(seed)
    z = scale * rng.standard_normal(shape)
    z = z - z.max(-1, keepdims=True)
    return (z - np.log(np.exp(z).sum(-1, keepdims=True))).astype(np.float32)


def transitions(seed, a, scale=0.5):
    return (scale * np.random.default_rng(seed).standard_normal((a, a))).astype(np.float32)


def gen_arpa(path, seed, order, letters='ABCDE', per_order=300, unk=-2.0):
    """a random order-``order`` ARPA model over the words of one to three ``letters`` (doubled letters included); higher
    n-grams extend lower ones by an older word"""
    from wav2letter_pytorch_amd.ngram_lm import ArpaLM
    rng = np.random.default_rng(seed)
    words = [''.join(w) for n in (1, 2) for w in itertools.product(letters, repeat=n)]
    words += sorted({''.join(rng.choice(list(letters), 3)) for _ in range(40)} - set(words))
    lines = {1: ['%.1f\t<unk>' % unk, '-99\t<s>\t%.5f' % -rng.uniform(0, 0.5), '%.5f\t</s>\t0' % -rng.uniform(0.3, 1.5)]}
    lines[1] += ['%.5f\t%s\t%.5f' % (-rng.uniform(0.3, 2.5), w, -rng.uniform(0, 0.6)) for w in words]
    grams = [(w,) for w in words + ['</s>']]
    for n in range(2, order + 1):
        cur = set()
        while len(cur) < per_order:
            base = grams[rng.integers(len(grams))]
            if base[0] != '<s>':
                cur.add(((['<s>'] + words)[rng.integers(len(words) + 1)],) + base)
        grams = sorted(cur)
        top = n == order
        lines[n] = ['%.5f\t%s' % (-rng.uniform(0.05, 1.5), ' '.join(gr)) + ('' if top else '\t%.5f' % -rng.uniform(0, 0.6))
                    for gr in grams]
    if order == 1:
        lines[1] = ['\t'.join(v.split('\t')[:2]) for v in lines[1]]
    text = '\\data\\\n' + ''.join('ngram %d=%d\n' % (n, len(lines[n])) for n in lines)
    for n in lines:
        text += '\n\\%d-grams:\n' % n + '\n'.join(lines[n]) + '\n'
    text += '\n\\end\\\n'
    path.write_text(text)
    return ArpaLM(str(path))


def word_scores(seed, n, t, labels, letters='ABCDE', p_space=0.3, boost=(3.0, 6.0), rival=1.5, p_double=0.3):
    """float32 log-softmax [n, t, labels] of bursts of a letter or a space, each burst with a rival label boosted almost as
    much, so that word choices are close calls; a letter burst is followed by a burst of the repeat label (index 0) with
    probability ``p_double``, so doubled letters occur inside words"""
    rng = np.random.default_rng(seed)
    a = len(labels)
    cand = [labels.index(c) for c in letters]
    space = labels.index(' ')
    logits = rng.standard_normal((n, t, a))
    for u in range(n):
        f, last = 0, -1
        while f < t:
            if last in cand and rng.random() < p_double:
                c = 0
            else:
                c = space if rng.random() < p_space else cand[rng.integers(len(cand))]
            r = cand[rng.integers(len(cand))]
            burst = int(rng.integers(1, 4))
            b = rng.uniform(*boost)
            logits[u, f:f + burst, c] += b
            logits[u, f:f + burst, r] += b - rng.uniform(0, rival)
            f += burst
            last = c
    z = logits - logits.max(-1, keepdims=True)
    return (z - np.log(np.exp(z).sum(-1, keepdims=True))).astype(np.float32)
