"""The device beam search with an ARPA n-gram model (w2l_ctc_beam_search with lm) against the host recursion with
``lm=lambda s: 10 ** arpa.score(s)``.

The models are generated at run time over short words of a few letters, so that the decoded strings are mostly
in-vocabulary and the LM changes what wins.  Every posterior is generated in float32 and widened exactly, as in
test_gpu_beam_search.py, and the cases stay where the host's float64 linear masses do not underflow."""
import functools
import itertools

import numpy as np
import pytest
import torch

from wav2letter_pytorch_amd.beam_search import (GPUPrefixBeamSearchLMDecoder, _beam_search_device, prefix_beam_search,
                                                prefix_beam_search_gpu)
from wav2letter_pytorch_amd.data.label_sets import english_labels
from wav2letter_pytorch_amd.ngram_lm import ArpaLM

pytestmark = pytest.mark.gpu

LETTERS = 'ABCDE'


def _gen_arpa(path, seed, order, letters=LETTERS, per_order=400, unk=-2.0):
    """a random order-``order`` ARPA model over the words of one to three ``letters``; higher n-grams extend lower ones by an
    older word, plus a few whose suffix is missing (closed by the loader)"""
    rng = np.random.default_rng(seed)
    words = [''.join(w) for n in (1, 2) for w in itertools.product(letters, repeat=n)]
    words += sorted({''.join(rng.choice(list(letters), 3)) for _ in range(40)})
    lines = {1: ['%.1f\t<unk>' % unk, '-99\t<s>\t%.5f' % -rng.uniform(0, 0.5), '%.5f\t</s>\t0' % -rng.uniform(0.3, 1.5)]}
    lines[1] += ['%.5f\t%s\t%.5f' % (-rng.uniform(0.3, 2.5), w, -rng.uniform(0, 0.6)) for w in words]
    grams = [(w,) for w in words + ['</s>']]
    for n in range(2, order + 1):
        cur = set()
        while len(cur) < per_order:
            base = grams[rng.integers(len(grams))]
            if base[0] != '<s>':
                cur.add(((['<s>'] + words)[rng.integers(len(words) + 1)],) + base)
        for _ in range(10):
            cur.add(tuple(words[i] for i in rng.integers(len(words), size=n)))
        grams = sorted(cur)
        top = n == order
        lines[n] = ['%.5f\t%s' % (-rng.uniform(0.05, 1.5), ' '.join(g)) + ('' if top else '\t%.5f' % -rng.uniform(0, 0.6))
                    for g in grams]
    if order == 1:
        lines[1] = ['\t'.join(x.split('\t')[:2]) for x in lines[1]]
    text = '\\data\\\n' + ''.join('ngram %d=%d\n' % (n, len(lines[n])) for n in lines)
    for n in lines:
        text += '\n\\%d-grams:\n' % n + '\n'.join(lines[n]) + '\n'
    text += '\n\\end\\\n'
    path.write_text(text)
    return ArpaLM(str(path))


def _posteriors(seed, n, t, labels, letters=LETTERS, p_blank=0.45, p_space=0.3, boost=(3.0, 6.0), rival=1.5, extra=()):
    """float32 [n, t, labels]: blank frames and bursts of a letter or a space, each burst with a rival label boosted almost
    as much, so that word choices are close calls"""
    rng = np.random.default_rng(seed)
    a = len(labels)
    cand = [labels.index(c) for c in letters] + [labels.index(c) for c in extra]
    space = labels.index(' ')
    logits = rng.standard_normal((n, t, a))
    for u in range(n):
        f = 0
        while f < t:
            if rng.random() < p_blank:
                logits[u, f, 0] += rng.uniform(*boost)
                f += 1
                continue
            c = space if rng.random() < p_space else cand[rng.integers(len(cand))]
            r = cand[rng.integers(len(cand))]
            burst = int(rng.integers(1, 3))
            b = rng.uniform(*boost)
            logits[u, f:f + burst, c] += b
            logits[u, f:f + burst, r] += b - rng.uniform(0, rival)
            f += burst
    e = np.exp(logits - logits.max(-1, keepdims=True))
    return (e / e.sum(-1, keepdims=True)).astype(np.float32)


def _weigh(lm):
    return functools.lru_cache(maxsize=None)(lambda s: 10 ** lm.score(s))


def _check_close(logw, w_host):
    assert w_host > 1e-250
    ref = np.log(w_host)
    assert abs(logw - ref) <= 1e-9 * max(1.0, abs(ref)), (logw, ref)


def _strip_score(lm, s, end_char='>'):
    return np.float32(lm.score(s.strip(' ' + end_char))) if s.replace(' ', '') else np.float32(0)


def _compare(lm, p, labels, k, alpha, beta, sizes=None, end_char='>'):
    """device vs host on every utterance: best string, log weight, and lm_log10 of every returned prefix"""
    x = torch.from_numpy(p).cuda()
    scores, lengths, idx, lmv = _beam_search_device(x, labels, 0, k, beta, 1e-3, end_char,
                                                    None if sizes is None else torch.tensor(sizes), False, lm=lm, alpha=alpha)
    weigh = _weigh(lm)
    bests = []
    for u in range(p.shape[0]):
        tn = p.shape[1] if sizes is None else sizes[u]
        best, w = prefix_beam_search(p[u, :tn].astype(np.float64), labels, lm=weigh, k=k, alpha=alpha, beta=beta,
                                     end_char=end_char, return_weights=True)
        found = [''.join(labels[j] for j in idx[u, r, :lengths[u, r]]) for r in range(k) if lengths[u, r] >= 0]
        assert found[0] == best, (u, found[0], best)
        _check_close(scores[u, 0], w)
        for r, s in enumerate(found):
            assert lmv[u, r].tobytes() == _strip_score(lm, s, end_char).tobytes(), (u, r, s, lmv[u, r])
        bests.append(best)
    return bests


CASES = [  # (order, alpha, beta, k, T)
    (1, 0.3, 5, 5, 60), (2, 1.0, 0, 16, 60), (3, 2.5, 5, 5, 50), (5, 1.0, 5, 32, 50),
    (2, 0.3, 0, 1, 80), (3, 1.0, 5, 16, 60), (5, 2.5, 0, 5, 40), (3, 0.3, 5, 32, 50),
]


@pytest.mark.parametrize('order,alpha,beta,k,t', CASES)
def test_matches_host(tmp_path, order, alpha, beta, k, t):
    lm = _gen_arpa(tmp_path / 'm.arpa', 100 + order, order)
    assert lm.order == order
    p = _posteriors(order * 7 + k, 6, t, english_labels)
    _compare(lm, p, english_labels, k, alpha, beta)


def test_nbest_matches_host_order(tmp_path):
    """the n-best list is the device's whole final beam in rank order; its first entry is the host's best"""
    lm = _gen_arpa(tmp_path / 'm.arpa', 7, 3)
    p = _posteriors(21, 4, 60, english_labels)
    lists = prefix_beam_search_gpu(p, english_labels, k=8, nbest=8, lm=lm, alpha=1.0, beta=2)
    best = prefix_beam_search_gpu(p, english_labels, k=8, lm=lm, alpha=1.0, beta=2)
    weigh = _weigh(lm)
    for u, (b, lst) in enumerate(zip(best, lists)):
        assert lst[0][0] == b == prefix_beam_search(p[u].astype(np.float64), english_labels, lm=weigh, k=8, alpha=1.0, beta=2)
        scores = [s for _, s in lst]
        assert all(x >= y for x, y in zip(scores, scores[1:]))


def test_sizes(tmp_path):
    lm = _gen_arpa(tmp_path / 'm.arpa', 3, 2)
    p = _posteriors(5, 6, 70, english_labels)
    _compare(lm, p, english_labels, 5, 1.0, 5, sizes=[70, 2, 17, 64, 45, 33])
    dec = GPUPrefixBeamSearchLMDecoder(str(tmp_path / 'm.arpa'), english_labels, k=5, alpha=1.0, beta=5)
    got = dec.decode(torch.from_numpy(p), sizes=torch.tensor([70, 2, 17, 64, 45, 33]))
    weigh = _weigh(dec.lm)
    assert got == [prefix_beam_search(p[n, :s].astype(np.float64), english_labels, lm=weigh, k=5, alpha=1.0, beta=5)
                   for n, s in enumerate([70, 2, 17, 64, 45, 33])]


def test_end_char_in_labels(tmp_path):
    labels = ['_', 'A', 'B', 'C', ' ', '>', "'"]
    lm = _gen_arpa(tmp_path / 'm.arpa', 11, 3, letters='ABC')
    closed = 0
    for seed in range(3):
        p = _posteriors(40 + seed, 6, 60, labels, letters='ABC', extra='>')
        bests = _compare(lm, p, labels, 8, 1.0, 2)
        closed += sum(b.endswith('>') for b in bests)
    assert closed > 0


def test_alpha_zero_is_the_lm_free_search(tmp_path):
    lm = _gen_arpa(tmp_path / 'm.arpa', 5, 3)
    p = torch.from_numpy(_posteriors(9, 8, 80, english_labels)).cuda()
    for k in (1, 5, 16):
        a = _beam_search_device(p, english_labels, 0, k, 5, 1e-3, '>', None, False)
        b = _beam_search_device(p, english_labels, 0, k, 5, 1e-3, '>', None, False, lm=lm, alpha=0.0)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()     # scores, lengths
        for u, r in zip(*np.nonzero(a[1] >= 0)):                                          # the valid labels of each slot
            assert a[2][u, r, :a[1][u, r]].tobytes() == b[2][u, r, :a[1][u, r]].tobytes()


def test_beam_width_changes(tmp_path):
    """decoder_test.py:44-59 with its lm (0.5 for 'A', else 1) as an ARPA bigram: p(A | <s>) = 10^-0.30103"""
    (tmp_path / 'a.arpa').write_text('\\data\\\nngram 1=4\nngram 2=2\n\n\\1-grams:\n-1\t<unk>\n-99\t<s>\t0\n0\t</s>\n'
                                     '-1\tA\t0\n\n\\2-grams:\n-0.30103\t<s> A\n0\tA </s>\n\n\\end\\\n')
    lm = ArpaLM(str(tmp_path / 'a.arpa'))
    assert lm.score('A') == float(np.float32(-0.30103))
    labels = ['_', 'A', ' ']
    samples = np.array([[0.8, 0.2, 0], [0.7, 0.3, 0], [0.6, 0.4, 0], [0.0, 0.0, 1]])
    weigh = _weigh(lm)
    assert prefix_beam_search(samples, labels, lm=weigh, k=25, alpha=1, beta=0) == ' '
    assert prefix_beam_search(samples, labels, lm=weigh, k=1, alpha=1, beta=0) == 'A '
    assert prefix_beam_search_gpu(samples, labels, lm=lm, k=25, alpha=1, beta=0) == ' '
    assert prefix_beam_search_gpu(samples, labels, lm=lm, k=1, alpha=1, beta=0) == 'A '
    dec = GPUPrefixBeamSearchLMDecoder(str(tmp_path / 'a.arpa'), labels, k=1, alpha=1, beta=0)
    assert dec.decode(samples) == 'A '


def test_lm_changes_the_decode(tmp_path):
    """a corpus where the LM changes the decoded string: the device follows the host on every utterance"""
    lm = _gen_arpa(tmp_path / 'm.arpa', 17, 3)
    p = _posteriors(33, 16, 60, english_labels)
    with_lm = _compare(lm, p, english_labels, 8, 2.5, 1)
    without = prefix_beam_search_gpu(p, english_labels, k=8, beta=1)
    changed = sum(a != b for a, b in zip(with_lm, without))
    assert changed >= 3, changed


def test_errors(tmp_path):
    lm = _gen_arpa(tmp_path / 'm.arpa', 1, 2)
    p = _posteriors(1, 1, 20, english_labels)
    with pytest.raises(ValueError, match='whitespace'):
        prefix_beam_search_gpu(p, english_labels[:-1] + ['\t'], lm=lm)
    with pytest.raises(TypeError):
        prefix_beam_search_gpu(p, english_labels, lm=lambda s: 1.0)
    with pytest.raises(Exception, match='beam width'):
        prefix_beam_search_gpu(p, english_labels, k=65, lm=lm)
