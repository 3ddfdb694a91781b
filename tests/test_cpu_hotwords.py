"""Hotword boosting of the CTC prefix beam search on the host (no GPU): the device's walk over the flat trie against the
definition (Lexicon.boost_chars), the boosted recursion against a brute-force enumeration of every alignment, the weight at which
a hotword overtakes a rival, the withdrawn credit of a partial word, the no-op cases, the command line and the constructors."""
import itertools
import math

import numpy as np
import pytest

from wav2letter_pytorch_amd.beam_search import prefix_beam_search
from wav2letter_pytorch_amd.data.label_sets import english_labels
from wav2letter_pytorch_amd.lexicon import Lexicon

HOT3 = ['abba', 'ab', 'bcc']                                     # a word, a prefix of it, a word with a doubled letter


def _h_by_definition(words, s, end_char):
    """the definition restated with startswith (not Lexicon's prefix set)"""
    parts = s.replace(end_char, ' ').split(' ')
    h = sum(len(p) for p in parts[:-1] if p in words)
    if parts[-1] and any(w.startswith(parts[-1]) for w in words):
        h += len(parts[-1])
    return h


def _device_rule(keys, vals, word, canon, seps, s):
    """the kernel's walk (hot_step / hot_chars of csrc/beam_lm.h) over the flat tables: h of the label string s"""
    table = dict(zip(keys.tolist(), vals.tolist()))
    node = depth = credit = 0
    for ch in s:
        c = canon[ch]
        if c in seps:
            if node > 0 and word[node] >= 0:
                credit += depth
            node = depth = 0
        elif node >= 0:
            node = table.get((node << 8) | c, -1)
            depth += 1
    return credit + (depth if node > 0 else 0)


def test_flat_trie_walk_matches_boost_chars():
    labels = ['_', 'a', 'b', 'c', ' ', '>', 'b']                 # five symbols, and a duplicate label
    hot = Lexicon(HOT3)
    keys, vals, word = hot.spelling_trie(labels, 0)
    assert hot.stats['unspellable'] == 0
    canon = {ch: labels.index(ch) for ch in labels}
    seps = {canon[' '], canon['>']}
    n = boosted = 0
    for length in range(7):
        for tup in itertools.product('abc >', repeat=length):
            s = ''.join(tup)
            want = _h_by_definition(HOT3, s, '>')
            assert hot.boost_chars(s) == want, s
            assert _device_rule(keys, vals, word, canon, seps, s) == want, s
            n += 1
            boosted += want > 0
    assert n == sum(5 ** i for i in range(7)) and 0 < boosted < n
    assert [hot.boost_chars(s) for s in ('', 'a', 'ab', 'abb', 'abba', 'abbab', 'ab ab', 'ab>bcc ', 'c ab')] == \
        [0, 1, 2, 3, 4, 0, 4, 5, 2]
    assert hot.boost_chars('ab|abb', end_char='|') == 5


def test_unspellable_hotwords_are_dropped_on_both_sides():
    """the search's oracle is boost_chars of the words the labels can spell, which are the words the flat trie holds"""
    labels = ['_', 'a', 'b', 'd', ' ']
    hot = Lexicon(['ab', 'da_', 'dax'])
    kept = hot.spellable(labels, 0)
    assert kept.words == ['ab'] and hot.stats['unspellable'] == 2
    assert hot.boost_chars('d') == 1 and kept.boost_chars('d') == 0
    assert Lexicon(['ab']).spellable(labels, 0).words == ['ab']
    with pytest.raises(ValueError, match='spelled'):
        Lexicon(['xyz']).spellable(labels, 0)
    p = np.array([[0.3, 0, 0, 0.7, 0], [1.0, 0, 0, 0, 0]])       # only '' and 'd' have mass
    got = prefix_beam_search(p, labels, k=30, beta=0, prune=0, return_weights=True, hotwords=hot, hotword_weight=3.0)
    assert got == ('d', 0.7)                                     # 'd' opens no hotword that the search could ever spell


# --------------------------------------------------------------------------------------- host recursion against brute force
BF_LABELS = ['_', 'a', 'b', 'c', ' ']
BF_T = 5


def _collapse(path, labels):
    out, prev = [], 0
    for l in path:
        if l != prev and l != 0:
            out.append(labels[l])
        prev = l
    return ''.join(out)


_BF_PATHS = list(itertools.product(range(5), repeat=BF_T))
_BF_STRINGS = [_collapse(p, BF_LABELS) for p in _BF_PATHS]


def _exact_masses(p):
    """float64 mass of every collapsed string: the sum over all 5^5 alignments"""
    mass = {}
    for path, s in zip(_BF_PATHS, _BF_STRINGS):
        mass[s] = mass.get(s, 0.0) + float(np.prod([p[t, l] for t, l in enumerate(path)]))
    return mass


def _n_words(s):
    """words closed by a space over these labels (beam_search._n_words: \\w+[\\s|>])"""
    return sum(1 for i, ch in enumerate(s) if ch == ' ' and i > 0 and s[i - 1] != ' ')


@pytest.mark.parametrize('seed', range(20))
def test_host_oracle_against_brute_force(seed):
    hot = Lexicon(HOT3)
    p = np.random.default_rng(seed).dirichlet(np.ones(5), size=BF_T)
    mass = _exact_masses(p)
    k = len(mass)                                                # nothing ever falls off the beam
    for gamma, beta in ((0.7, 0), (2.5, 0), (-0.9, 0), (0.7, 1.5)):
        key = {s: mass[s] * (_n_words(s) + 1) ** beta * math.exp(gamma * hot.boost_chars(s)) for s in mass}
        want = max(key, key=lambda s: key[s])
        got, w = prefix_beam_search(p, BF_LABELS, lm=None, k=k, beta=beta, prune=0, return_weights=True, hotwords=hot,
                                    hotword_weight=gamma)
        assert got == want, (gamma, beta, got, want)
        assert abs(w - key[want]) <= 1e-12 * key[want], (w, key[want])


def test_boost_changes_a_decode():
    """some seeds' best string changes under the boost, so the test above is not vacuous"""
    hot = Lexicon(HOT3)
    changed = 0
    for seed in range(20):
        p = np.random.default_rng(seed).dirichlet(np.ones(5), size=BF_T)
        changed += (prefix_beam_search(p, BF_LABELS, k=400, beta=0, prune=0)
                    != prefix_beam_search(p, BF_LABELS, k=400, beta=0, prune=0, hotwords=hot, hotword_weight=2.5))
    assert changed >= 3, changed


# -------------------------------------------------------------------------------------------------------------- threshold
def test_hotword_overtakes_its_rival_at_the_predicted_weight():
    """'ac ' has r times the mass of 'ab '; 'ab' is a hotword (d = 2 characters more credit): the best string flips between
    gamma = 0.5 ln(r) / d and 2 ln(r) / d, at every beam width (the partial credit of 'ab' is the same 2 one frame earlier)"""
    labels = ['_', 'a', 'b', 'c', ' ']
    r, d = 3.0, 2
    p = np.array([[0, 1, 0, 0, 0], [0, 0, 1 / (1 + r), r / (1 + r), 0], [0, 0, 0, 0, 1.0]])
    hot = Lexicon(['ab'])
    assert hot.boost_chars('ab ') - hot.boost_chars('ac ') == d
    for k in (1, 2, 5):
        assert prefix_beam_search(p, labels, k=k, beta=0, prune=0) == 'ac '
        lo, w_lo = prefix_beam_search(p, labels, k=k, beta=0, prune=0, return_weights=True, hotwords=hot,
                                      hotword_weight=0.5 * math.log(r) / d)
        hi, w_hi = prefix_beam_search(p, labels, k=k, beta=0, prune=0, return_weights=True, hotwords=hot,
                                      hotword_weight=2 * math.log(r) / d)
        assert (lo, hi) == ('ac ', 'ab ')
        assert abs(w_lo - r / (1 + r)) <= 1e-12                  # no credit: the plain mass
        assert abs(w_hi - r * r / (1 + r)) <= 1e-12              # 1 / (1 + r) * exp(2 * ln(r) / d * d)
    # a negative weight pushes the hotword down instead
    p2 = np.array([[0, 1, 0, 0, 0], [0, 0, r / (1 + r), 1 / (1 + r), 0], [0, 0, 0, 0, 1.0]])
    assert prefix_beam_search(p2, labels, k=2, beta=0, prune=0) == 'ab '
    assert prefix_beam_search(p2, labels, k=2, beta=0, prune=0, hotwords=hot, hotword_weight=-2 * math.log(r) / d) == 'ac '


# ------------------------------------------------------------------------------------------------------- withdrawn credit
def test_partial_credit_is_withdrawn_when_the_word_closes_as_something_else():
    hot = Lexicon(['abba'])
    assert [hot.boost_chars(s) for s in ('a', 'ab', 'abb', 'abb ', 'abb>', 'abba', 'abba ', 'abbab', 'abb a')] == \
        [1, 2, 3, 0, 0, 4, 4, 0, 1]
    labels = ['_', 'a', 'b', ' ']
    one = lambda i: [1.0 if j == i else 0.0 for j in range(4)]   # noqa: E731
    p = np.array([one(1), one(2), one(0), one(2), one(3)])       # a b _ b ' '
    gamma = 0.7
    for k in (1, 4):
        live = prefix_beam_search(p[:4], labels, k=k, beta=0, prune=0, return_weights=True, hotwords=hot, hotword_weight=gamma)
        assert live[0] == 'abb' and abs(live[1] - math.exp(3 * gamma)) <= 1e-12        # mass 1, three characters on credit
        closed = prefix_beam_search(p, labels, k=k, beta=0, prune=0, return_weights=True, hotwords=hot, hotword_weight=gamma)
        assert closed == ('abb ', 1.0)                           # ... and none once 'abb' is closed
    whole = np.array([one(1), one(2), one(0), one(2), one(1), one(3)])
    got = prefix_beam_search(whole, labels, k=2, beta=0, prune=0, return_weights=True, hotwords=hot, hotword_weight=gamma)
    assert got[0] == 'abba ' and abs(got[1] - math.exp(4 * gamma)) <= 1e-12


# -------------------------------------------------------------------------------------------------------------------- no-op
def _asr_sample():
    s = np.zeros((10, len(english_labels)))
    s[0, 2] = 0.5
    s[1, 20] = 0.5
    s[2, 19] = 0.5
    s[3:, 0] = 0.5
    return s


def _bits(result):
    return (result[0], float(result[1]).hex()) if isinstance(result, tuple) else result


def test_no_hotwords_and_weight_zero_change_nothing():
    def the_lm(s):
        return 0.5 if s == 'A' else 1
    ab = np.array([[0.8, 0.2, 0, 0], [0.6, 0.4, 0, 0]])
    width = np.array([[0.8, 0.2, 0], [0.7, 0.3, 0], [0.6, 0.4, 0], [0.0, 0.0, 1]])
    cases = [  # (posteriors, labels, keywords, the known answer of tests/test_beam_search.py)
        (_asr_sample(), english_labels, dict(), 'ASR'),
        (_asr_sample(), english_labels, dict(return_weights=True), None),
        (ab, ['_', 'A', 'B', ' '], dict(blank_index=0, return_weights=True), ('A', 0.52)),
        (width, ['_', 'A', ' '], dict(lm=the_lm, k=25, alpha=1, beta=0), ' '),
        (width, ['_', 'A', ' '], dict(lm=the_lm, k=1, alpha=1, beta=0), 'A '),
        (width, ['_', 'A', ' '], dict(lm=the_lm, k=25, alpha=1, beta=0, return_weights=True), None),
        (width, ['_', 'A', ' '], dict(k=3, beta=5, return_weights=True), None),
    ]
    changed = 0
    for p, labels, kw, known in cases:
        plain = prefix_beam_search(p, labels, **kw)
        assert known is None or plain == known
        assert _bits(prefix_beam_search(p, labels, hotwords=None, hotword_weight=3.0, **kw)) == _bits(plain)
        for hot in (Lexicon(['A', 'AS', 'SR']), ['A', 'B'], iter(['AA'])):
            assert _bits(prefix_beam_search(p, labels, hotwords=hot, hotword_weight=0, **kw)) == _bits(plain)
        changed += _bits(prefix_beam_search(p, labels, hotwords=['A', 'AS'], hotword_weight=1.5, **kw)) != _bits(plain)
    assert changed >= 1                                          # (a weight does change ('A', 0.52): h('A') = 1)
    with pytest.raises(ValueError, match='finite'):
        prefix_beam_search(ab, ['_', 'A', 'B', ' '], hotwords=['A'], hotword_weight=float('inf'))


# ------------------------------------------------------------------------------------------------------------------- config
def test_command_line_rules():
    from wav2letter_pytorch_amd import test as T
    base = ['model_path=a.ckpt', 'data.test_manifest=m.csv']
    cfg = T.build_config(base + ['decoder=beam', 'hotwords_path=words.txt'])
    name, kw = T.decoder_spec(cfg, True)
    assert name == 'GPUPrefixBeamSearchDecoder' and kw['hotwords'] == 'words.txt' and kw['hotword_weight'] == 1.0
    assert 'lexicon' not in kw
    cfg = T.build_config(base + ['decoder=beam_lm', 'lm_path=lm.arpa', 'hotwords_path=words.txt', 'hotword_weight=-0.25',
                                 'lexicon_from_lm=true', 'word_times=true'])
    name, kw = T.decoder_spec(cfg, False)
    assert name == 'GPUPrefixBeamSearchLMDecoder' and kw['hotwords'] == 'words.txt' and kw['hotword_weight'] == -0.25
    assert kw['lexicon'] == 'lm' and kw['lm_path'] == 'lm.arpa' and cfg.word_times
    cfg = T.build_config(base + ['decoder=beam', 'hotwords_path=words.txt', 'hotword_weight=0'])
    assert T.decoder_spec(cfg, True)[1]['hotword_weight'] == 0.0
    for dec in (['decoder=beam'], ['decoder=beam_lm', 'lm_path=lm.arpa'], ['decoder=beam', 'lexicon_path=w.txt']):
        kw = T.decoder_spec(T.build_config(base + dec), True)[1]  # no hotwords: today's dictionaries
        assert 'hotwords' not in kw and 'hotword_weight' not in kw
        assert set(kw) - {'lexicon'} == {'lm_path', 'labels', 'k', 'alpha', 'beta', 'prune', 'log_probs'}
    assert T.decoder_spec(T.build_config(base), True) == ('GreedyDecoder', dict(labels=T.build_config(base).model.labels))
    for key in ('hotwords_path=words.txt', 'hotword_weight=2'):
        with pytest.raises(SystemExit, match=key.split('=')[0]):
            T.build_config(base + ['decoder=greedy', key])
        with pytest.raises(SystemExit, match=key.split('=')[0]):
            T.build_config(base + [key])
    with pytest.raises(SystemExit, match='without hotwords_path'):
        T.build_config(base + ['decoder=beam', 'hotword_weight=2'])
    with pytest.raises(SystemExit, match='not a number'):
        T.build_config(base + ['decoder=beam', 'hotwords_path=words.txt', 'hotword_weight=much'])
    with pytest.raises(SystemExit, match='not finite'):
        T.build_config(base + ['decoder=beam', 'hotwords_path=words.txt', 'hotword_weight=inf'])
    asg = base + ['model.criterion=asg']
    with pytest.raises(SystemExit, match='not built for ASG'):
        T.build_config(asg + ['decoder=asg_beam', 'hotwords_path=words.txt'])
    with pytest.raises(SystemExit, match='not built for ASG'):
        T.build_config(asg + ['decoder=asg_beam_lm', 'lm_path=lm.arpa', 'hotwords_path=words.txt', 'hotword_weight=1'])
    # not a beam.* option: the list of those and its error text are as they were
    with pytest.raises(SystemExit) as err:
        T.build_config(base + ['decoder=beam', 'hotwords_path=words.txt', 'beam.hotword_weight=2'])
    assert str(err.value) == "unknown beam option(s) ['hotword_weight']: beam.k, beam.alpha, beam.beta, beam.prune"
    assert T.BEAM_DEFAULTS == dict(k=5, alpha=0.3, beta=5, prune=1e-3)


def test_decoder_constructors(tmp_path):
    from wav2letter_pytorch_amd.beam_search import GPUPrefixBeamSearchDecoder, GPUPrefixBeamSearchLMDecoder
    arpa = tmp_path / 'm.arpa'
    arpa.write_text('\\data\\\nngram 1=4\n\n\\1-grams:\n-1\t<unk>\n-99\t<s>\n-0.5\t</s>\n-1\tA\n\n\\end\\\n')
    (tmp_path / 'w.txt').write_text('# names\nABBA\nBED b e d\n')
    for cls, lm_path in ((GPUPrefixBeamSearchDecoder, None), (GPUPrefixBeamSearchLMDecoder, str(arpa))):
        d = cls(lm_path, english_labels)
        assert d.hotwords is None
        d = cls(lm_path, english_labels, hotwords=str(tmp_path / 'w.txt'))
        assert d.hotwords.words == ['ABBA', 'BED'] and d.hotword_weight == 1.0       # the conventional default
        d = cls(lm_path, english_labels, hotwords=(w for w in ['AB', 'ABBA', 'AB']), hotword_weight=-0.5)
        assert d.hotwords.words == ['AB', 'ABBA'] and d.hotword_weight == -0.5 and d.hotwords.stats['duplicates'] == 1
        hot = Lexicon(['BED', 'déjà'])
        d = cls(lm_path, english_labels, hotwords=hot, lexicon=Lexicon(['A']))
        assert d.hotwords is hot and hot.stats['unspellable'] == 1 and d.lexicon.words == ['A']
        with pytest.raises(ValueError, match='not a word'):
            cls(lm_path, english_labels, hotwords=['NEW YORK'])
        with pytest.raises(ValueError, match='spelled'):
            cls(lm_path, english_labels, hotwords=['déjà', 'x_y'])
        with pytest.raises(ValueError, match='finite'):
            cls(lm_path, english_labels, hotwords=['A'], hotword_weight=float('nan'))
