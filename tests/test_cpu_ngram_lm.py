"""ngram_lm.ArpaLM on the host: hand-computed float32 scores, malformed files, and a NumPy restatement of the device walk
(the reverse-suffix entries and their hash keys) that must agree bit for bit with score().  No device work."""
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

from wav2letter_pytorch_amd.ngram_lm import BOS, EOS, UNK, ArpaLM, table_capacity

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f = np.float32


def _fsum(*vals):
    """float32 running sum, left to right"""
    acc = f(vals[0])
    for v in vals[1:]:
        acc = f(acc + f(v))
    return float(acc)


def _write(tmp_path, name, text):
    p = tmp_path / name
    p.write_text(text)
    return str(p)


BIGRAM = r"""some preamble a tool writes
\data\
ngram 1=5
ngram 2=3

\1-grams:
-1.0	<unk>
-99	<s>	-0.5
-0.7	</s>
-0.4	a	-0.3
-0.6 b -0.2

\2-grams:
-0.2	<s> a
-0.3	a b
-0.1	b </s>

\end\
"""

UNIGRAMS_4 = [('-2.0', '<unk>', None), ('-99', '<s>', '-0.25'), ('-1.0', '</s>', None), ('-0.5', 'a', '-0.11'),
              ('-0.6', 'b', '-0.12'), ('-0.7', 'c', '-0.13')]
BIGRAMS_4 = [('-0.3', '<s> a', '-0.21'), ('-0.35', 'a b', '-0.22'), ('-0.4', 'b c', '-0.23')]
TRIGRAMS_4 = [('-0.15', '<s> a b', '-0.31'), ('-0.2', 'a b c', '-0.32')]
FOURGRAMS_4 = [('-0.05', '<s> a b c', None)]


def _arpa(sections):
    out = ['\\data\\']
    out += ['ngram %d=%d' % (n + 1, len(s)) for n, s in enumerate(sections)]
    for n, sec in enumerate(sections):
        out += ['', '\\%d-grams:' % (n + 1)]
        top = n == len(sections) - 1
        for p, words, bo in sec:
            out.append('\t'.join([p, words] + ([bo] if bo is not None and not top else [])))
    out += ['', '\\end\\', '']
    return '\n'.join(out)


def test_bigram_backoff(tmp_path):
    lm = ArpaLM(_write(tmp_path, 'bi.arpa', BIGRAM))
    assert lm.order == 2 and lm.words[:5] == ['<unk>', '<s>', '</s>', 'a', 'b'] and not lm.warnings
    assert lm.score('a b') == _fsum(-0.2, -0.3, -0.1)
    assert lm.score('b a') == _fsum(_fsum(-0.6, -0.5), _fsum(-0.4, -0.2), _fsum(-0.7, -0.3))
    assert lm.score('') == _fsum(-0.7, -0.5)
    assert lm.score('  a   b ') == lm.score('a b')
    assert lm.score('a b', bos=False) == _fsum(-0.4, -0.3, -0.1)
    assert lm.score('a b', bos=False, eos=False) == _fsum(-0.4, -0.3)
    assert lm.score('b', eos=False) == _fsum(-0.6, -0.5)


def test_oov_is_unk(tmp_path):
    lm = ArpaLM(_write(tmp_path, 'bi.arpa', BIGRAM))
    assert lm.score('zz') == _fsum(_fsum(-1.0, -0.5), -0.7)
    assert lm.score('a zz') == _fsum(-0.2, _fsum(-1.0, -0.3), -0.7)
    assert lm.score('zz') == lm.score('<unk>')


@pytest.mark.parametrize('order', [3, 4])
def test_backoff_chains(tmp_path, order):
    secs = [UNIGRAMS_4, BIGRAMS_4, TRIGRAMS_4, FOURGRAMS_4][:order]
    lm = ArpaLM(_write(tmp_path, 'm.arpa', _arpa(secs)))
    assert lm.order == order and lm.stats['context_only'] == 0
    if order == 4:
        # <s> a b c: the 4-gram; </s> after (a b c): unigram + bo(c) + bo(b c) + bo(a b c)
        assert lm.score('a b c') == _fsum(-0.3, -0.15, -0.05, _fsum(-1.0, -0.13, -0.23, -0.32))
    else:
        # c after (<s> a b) on a trigram model: a b c
        assert lm.score('a b c') == _fsum(-0.3, -0.15, -0.2, _fsum(-1.0, -0.13, -0.23))
    # a after (b a <s>): three backoffs, one of them absent when order == 3 (the history holds two words)
    tail = [-0.12, -0.22, -0.31] if order == 4 else [-0.12, -0.22]
    eos = _fsum(-1.0, -0.11) if order == 4 else _fsum(-1.0, -0.11, 0.0)
    assert lm.score('a b a') == _fsum(-0.3, -0.15, _fsum(-0.5, *tail), eos)
    # OOV in the middle of a chain
    assert lm.score('a zz', eos=False) == _fsum(-0.3, _fsum(-2.0, -0.11, -0.21))


def test_missing_unk_is_minus_100(tmp_path):
    secs = [UNIGRAMS_4[1:], BIGRAMS_4]
    lm = ArpaLM(_write(tmp_path, 'nounk.arpa', _arpa(secs)))
    assert lm.warnings and '<unk>' in lm.warnings[0]
    assert lm.score('zz', eos=False) == _fsum(-100.0, -0.25)
    assert lm.flat_tables()['prob'][UNK] == f(-100.0)


def test_context_only_suffix(tmp_path):
    # 'x y z' has no 'y z': suffix closure inserts it as context-only; it must not score as a bigram
    uni = UNIGRAMS_4[:3] + [('-0.9', 'x', '-0.01'), ('-0.8', 'y', '-0.02'), ('-0.75', 'z', '-0.03')]
    bi = [('-0.5', 'x y', '-0.04'), ('-0.45', '<s> x', '-0.05')]
    tri = [('-0.1', 'x y z', None)]
    lm = ArpaLM(_write(tmp_path, 'ctx.arpa', _arpa([uni, bi, tri])))
    assert lm.stats['context_only'] == 1 and lm.stats['counts'] == [6, 2, 1]
    y, z = lm.vocab['y'], lm.vocab['z']
    assert np.isnan(lm.ngrams[1][(y, z)][0]) and lm.ngrams[1][(y, z)][1] == 0.0
    assert lm.score('x y z', eos=False) == _fsum(-0.45, _fsum(-0.5, -0.05), -0.1)
    assert lm.score('y z', eos=False) == _fsum(_fsum(-0.8, -0.25), _fsum(-0.75, -0.02))
    flat = lm.flat_tables()
    assert int(np.isnan(flat['prob']).sum()) == 1


def test_gzip(tmp_path):
    p = tmp_path / 'bi.arpa.gz'
    with gzip.open(p, 'wt') as fh:
        fh.write(BIGRAM)
    plain = ArpaLM(_write(tmp_path, 'bi.arpa', BIGRAM))
    lm = ArpaLM(str(p))
    for s in ('a b', 'b a', 'zz a', ''):
        assert lm.score(s) == plain.score(s)


# -------------------------------------------------------------------------------------------------------- malformed files
def _bad(tmp_path, text, match, binary=False):
    p = tmp_path / 'bad.arpa'
    if binary:
        p.write_bytes(text)
    else:
        p.write_text(text)
    with pytest.raises(ValueError, match=match):
        ArpaLM(str(p))


def test_malformed_files(tmp_path):
    _bad(tmp_path, BIGRAM.replace('ngram 2=3', 'ngram 2=4'), r'line \d+.*announces 4')
    _bad(tmp_path, BIGRAM.replace('ngram 1=5', 'ngram 1=4'), r'line \d+.*more than the 4')
    _bad(tmp_path, BIGRAM.replace('-0.1\tb </s>', '-0.1\ta b'), r'line 16: duplicate 2-gram')
    _bad(tmp_path, BIGRAM.replace('-0.6 b -0.2', '-0.6 a -0.2'), r'line 11: duplicate unigram')
    _bad(tmp_path, BIGRAM.split('\\2-grams:')[0], r'truncated')
    _bad(tmp_path, BIGRAM.replace('\\end\\', ''), r'truncated')
    _bad(tmp_path, '\\data\\\n' + ''.join('ngram %d=1\n' % n for n in range(1, 8)), r'line 8: order 7 > 6')
    _bad(tmp_path, BIGRAM.replace('-0.3\ta b', '-0.3\ta b -0.1 -0.2'), r'line \d+: a 2-gram line')
    _bad(tmp_path, BIGRAM.replace('-0.1\tb </s>', '-0.1\tb q'), r'not a unigram')
    _bad(tmp_path, b'mmap lm http://kheafield.com/code format version 5\n\x00\x01\x02', 'convert to ARPA', binary=True)
    gz = tmp_path / 'bin.gz'
    with gzip.open(gz, 'wb') as fh:
        fh.write(b'mmap lm http://kheafield.com/code\x00')
    with pytest.raises(ValueError, match='convert to ARPA'):
        ArpaLM(str(gz))


# ------------------------------------------------------------------------------------------ the device layout, restated
def random_arpa(seed, order=5, vocab=40, per_order=300, extra=20):
    """a random ARPA model: n-grams of order n extend n-1-grams by an older word (suffix-closed), plus ``extra`` random
    n-grams per order whose suffixes may be missing (the loader closes them)"""
    rng = np.random.default_rng(seed)
    words = ['w%d' % i for i in range(vocab)]
    uni = [('-1.5', '<unk>', '0')] + [('-99', '<s>', '%.4f' % -rng.uniform(0, 1))] + [('-1.2', '</s>', None)]
    uni += [('%.6f' % -rng.uniform(0.3, 3), w, '%.6f' % -rng.uniform(0, 1)) for w in words]
    secs = [uni]
    grams = [(w,) for w in words + ['</s>']]
    ctxw = words + ['<s>']
    for n in range(2, order + 1):
        cur = set()
        while len(cur) < per_order:
            base = grams[rng.integers(len(grams))]
            if base[0] == '<s>':
                continue
            cur.add((ctxw[rng.integers(len(ctxw))],) + base)
        for _ in range(extra):
            g = tuple(ctxw[rng.integers(len(ctxw))] for _ in range(n - 1)) + (words[rng.integers(vocab)],)
            if '<s>' not in g[1:]:
                cur.add(g)
        cur = sorted(cur)
        secs.append([('%.6f' % -rng.uniform(0.05, 2), ' '.join(g), '%.6f' % -rng.uniform(0, 1)) for g in cur])
        grams = cur
    return _arpa(secs)


def walk_scores(lm, sentences):
    """ArpaLM.score(s) for every s, as w2l_ctc_beam_search computes it with lm: float32 state per sentence (last order-1 word
    ids, their context backoffs), q by the reverse-suffix walk over flat_tables() (keys looked up exactly), vectorised"""
    flat = lm.flat_tables()
    P, BO = flat['prob'], flat['bo']
    order = lm.order
    srt = np.argsort(flat['keys'])
    K, V = flat['keys'][srt], flat['vals'][srt]
    S = len(sentences)
    ids = [[lm.vocab.get(w, UNK) for w in s.split()] for s in sentences]
    L = max(1, max(len(x) for x in ids))
    W = np.full((S, L), -1, dtype=np.int64)
    for i, x in enumerate(ids):
        W[i, :len(x)] = x
    nc = max(order - 1, 1)
    ctx = np.zeros((S, nc), dtype=np.int64)
    cbo = np.zeros((S, nc), dtype=np.float32)
    m = np.full(S, min(1, order - 1), dtype=np.int64)
    if order > 1:
        ctx[:, 0] = BOS
        cbo[:, 0] = BO[BOS]

    def lookup(e, w):
        key = (e.astype(np.uint64) << np.uint64(32)) | w.astype(np.uint64)
        pos = np.minimum(np.searchsorted(K, key), len(K) - 1)
        hit = K[pos] == key if len(K) else np.zeros(len(key), dtype=bool)
        return hit, np.where(hit, V[pos] if len(K) else 0, -1)

    def q(w, ctx, cbo, m):
        e = w.copy()
        prob = P[e].copy()
        nbo = np.zeros((S, order), dtype=np.float32)
        nbo[:, 0] = BO[e]
        j = np.zeros(S, dtype=np.int64)
        depth = np.ones(S, dtype=np.int64)
        alive = np.ones(S, dtype=bool)
        for i in range(order - 1):
            act = alive & (i < m)
            hit, e2 = lookup(e, ctx[:, i])
            hit &= act
            alive &= hit | ~act
            e = np.where(hit, e2, e)
            depth = np.where(hit, i + 2, depth)
            p = P[e]
            real = hit & ~np.isnan(p)
            prob = np.where(real, p, prob)
            j = np.where(real, i + 1, j)
            nbo[:, i + 1] = np.where(hit, BO[e], 0)
        val = prob.astype(np.float32)
        for i in range(order - 1):
            val = np.where((i >= j) & (i < m), val + cbo[:, i], val)
        m2 = np.minimum(m + 1, order - 1)
        ctx2 = np.zeros_like(ctx)
        cbo2 = np.zeros_like(cbo)
        if order > 1:
            ctx2[:, 1:] = ctx[:, :-1]
            ctx2[:, 0] = w
            for i in range(order - 1):
                cbo2[:, i] = np.where((i < m2) & (i < depth), nbo[:, i], 0)
        return val.astype(np.float32), ctx2, cbo2, m2

    total = np.zeros(S, dtype=np.float32)
    for t in range(L):
        on = W[:, t] >= 0
        val, c2, b2, m2 = q(np.where(on, W[:, t], 0), ctx, cbo, m)
        total = np.where(on, total + val, total)
        ctx = np.where(on[:, None], c2, ctx)
        cbo = np.where(on[:, None], b2, cbo)
        m = np.where(on, m2, m)
    val, _, _, _ = q(np.full(S, EOS), ctx, cbo, m)
    return (total + val).astype(np.float32)


@pytest.mark.parametrize('order', [5, 2, 1])
def test_walk_over_flat_tables_matches_score(tmp_path, order):
    if order == 1:
        lm = ArpaLM(_write(tmp_path, 'u.arpa', _arpa([UNIGRAMS_4])))
    else:
        lm = ArpaLM(_write(tmp_path, 'r.arpa', random_arpa(order, order=order)))
    assert lm.order == order
    if order == 5:
        assert lm.stats['context_only'] > 0
    rng = np.random.default_rng(order)
    words = lm.words[3:] + ['oov1', 'oov2']
    sents = [' '.join(words[i] for i in rng.integers(len(words), size=rng.integers(0, 13))) for _ in range(3000)]
    # sentences that follow the model's own n-grams, so that long matches occur
    for g in list(lm.ngrams[-1])[:500]:
        sents.append(' '.join(lm.words[w] for w in g if w not in (BOS, EOS)))
    got = walk_scores(lm, sents)
    ref = np.array([lm.score(s) for s in sents], dtype=np.float32)
    assert got.tobytes() == ref.tobytes(), np.nonzero(got != ref)[0][:10]


def test_flat_tables_layout(tmp_path):
    lm = ArpaLM(_write(tmp_path, 'r.arpa', random_arpa(3, order=4, per_order=50)))
    flat = lm.flat_tables()
    V = flat['vocab']
    assert V == len(lm.words) and len(flat['prob']) == sum(len(d) for d in lm.ngrams)
    keys = flat['keys']
    assert len(np.unique(keys)) == len(keys) and table_capacity(len(keys)) >= 2 * len(keys)
    # key = parent entry << 32 | oldest word, parent = the entry of the n-gram without its oldest word
    assert np.array_equal(keys >> np.uint64(32), flat['parent'][V:].astype(np.uint64))
    assert (flat['parent'][:V] == -1).all()


def test_spelling_trie(tmp_path):
    lm = ArpaLM(_write(tmp_path, 'bi.arpa', BIGRAM.replace('ngram 1=5', 'ngram 1=7').replace(
        '-0.6 b -0.2', '-0.6 b -0.2\n-0.9 ab\n-0.9 a_b')))
    labels = ['_', 'a', 'b', ' ', 'a']
    keys, vals, word = lm.spelling_trie(labels, 0)
    child = {int(k): int(v) for k, v in zip(keys, vals)}
    a = child[(0 << 8) | 1]
    ab = child[(a << 8) | 2]
    assert word[a] == lm.vocab['a'] and word[ab] == lm.vocab['ab'] and word[child[2]] == lm.vocab['b']
    assert len(word) == 4                            # root, a, ab, b: 'a_b' holds the blank's character, '<s>' a '<'


# ------------------------------------------------------------------------------------------------------- configuration
def test_target_resolves(tmp_path):
    from wav2letter_pytorch_amd.beam_search import GPUPrefixBeamSearchLMDecoder
    from wav2letter_pytorch_amd.config import instantiate, to_cfg
    from wav2letter_pytorch_amd.data.label_sets import english_labels
    path = _write(tmp_path, 'bi.arpa', BIGRAM)
    cfg = to_cfg({'_target_': 'decoder.GPUPrefixBeamSearchLMDecoder', 'lm_path': path, 'labels': english_labels, 'k': 16,
                  'alpha': 0.8, 'beta': 2, 'prune': 1e-4})
    dec = instantiate(cfg)
    assert type(dec) is GPUPrefixBeamSearchLMDecoder
    assert (dec.k, dec.alpha, dec.beta, dec.prune, dec.log_probs) == (16, 0.8, 2, 1e-4, False)
    assert dec.lm.score('a b') == _fsum(-0.2, -0.3, -0.1)
    assert GPUPrefixBeamSearchLMDecoder(None, english_labels).lm is None
    from wav2letter_pytorch_amd import decoder
    assert decoder.GPUPrefixBeamSearchLMDecoder is GPUPrefixBeamSearchLMDecoder


def test_dropin_name_resolves(tmp_path):
    path = _write(tmp_path, 'bi.arpa', BIGRAM)
    code = r"""
import sys
import decoder
from wav2letter_pytorch_amd import beam_search
from wav2letter_pytorch_amd.config import instantiate
assert decoder.GPUPrefixBeamSearchLMDecoder is beam_search.GPUPrefixBeamSearchLMDecoder
dec = instantiate({'_target_': 'decoder.GPUPrefixBeamSearchLMDecoder', 'lm_path': sys.argv[1], 'labels': ['_', 'a', 'b', ' ']})
assert type(dec) is decoder.GPUPrefixBeamSearchLMDecoder and dec.lm.order == 2
print('dropin ok')
"""
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(ROOT, 'dropin'), ROOT]))
    out = subprocess.run([sys.executable, '-c', code, path], env=env, cwd=ROOT, capture_output=True, text=True, timeout=240)
    assert out.returncode == 0 and 'dropin ok' in out.stdout, out.stderr[-3000:]
