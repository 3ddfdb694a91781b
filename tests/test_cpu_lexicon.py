"""The lexicon constraint of the CTC prefix beam search on the host (no GPU): the word-list loader, the flat spelling trie
against the definition (Lexicon.allows / complete), the constrained recursion against a brute-force enumeration of every
alignment, and the command-line rules."""
import gzip
import itertools

import numpy as np
import pytest

from wav2letter_pytorch_amd.beam_search import prefix_beam_search
from wav2letter_pytorch_amd.data.label_sets import english_labels
from wav2letter_pytorch_amd.lexicon import Lexicon
from wav2letter_pytorch_amd.ngram_lm import ArpaLM

SMALL_ARPA = ('\\data\\\nngram 1=6\nngram 2=2\n\n\\1-grams:\n-1\t<unk>\n-99\t<s>\t0\n-0.5\t</s>\n-1\tA\t0\n-1.2\tAB\t0\n'
              "-1.5\tB'C\t0\n\n\\2-grams:\n-0.30103\t<s> A\n-0.2\tA </s>\n\n\\end\\\n")


# ------------------------------------------------------------------------------------------------------------------ parsing
def test_parsing(tmp_path):
    text = '# a comment\nhello h e l l o\n\nworld\tw o r l d\n   \nhello h e l o\n  #indented comment\nab\n'
    plain = tmp_path / 'words.txt'
    plain.write_text(text)
    packed = tmp_path / 'words.txt.gz'
    with gzip.open(packed, 'wt', encoding='utf-8') as f:
        f.write(text)
    for src in (plain, str(plain), packed):
        lex = Lexicon(src)
        assert lex.words == ['hello', 'world', 'ab']             # the first token of each line, first occurrence kept
        assert lex.stats['duplicates'] == 1 and lex.stats['words'] == 3 and len(lex) == 3
        assert 'hello' in lex and 'h' not in lex
    lex = Lexicon(iter(['ab', 'abba', 'ab']))
    assert lex.words == ['ab', 'abba'] and lex.stats['duplicates'] == 1
    with pytest.raises(ValueError):
        Lexicon(['two words'])
    with pytest.raises(ValueError):
        Lexicon([''])


def test_unspellable_and_empty():
    labels = ['_', 'a', 'b', ' ', 'a']                           # the second 'a' spells with index 1
    lex = Lexicon(['ab', 'abc', 'a_b', 'ba'])
    keys, vals, word = lex.spelling_trie(labels, 0)
    assert lex.stats['unspellable'] == 2                         # 'abc': no label c; 'a_b': the blank's character
    assert keys.dtype == np.uint64 and vals.dtype == np.int32 and word.dtype == np.int32
    assert sorted(keys.tolist()) == sorted([(0 << 8) | 1, (1 << 8) | 2, (0 << 8) | 2, (3 << 8) | 1])
    assert word.tolist() == [-1, -1, 0, -1, 3] and len(word) == len(keys) + 1
    assert lex.spelling_trie(labels, 0) is lex.spelling_trie(labels, 0)
    with pytest.raises(ValueError, match='spelled'):
        Lexicon(['xyz', 'q']).spelling_trie(labels, 0)


def test_from_lm(tmp_path):
    (tmp_path / 'm.arpa').write_text(SMALL_ARPA)
    lm = ArpaLM(str(tmp_path / 'm.arpa'))
    lex = Lexicon.from_lm(lm)
    assert lex.words == ['A', 'AB', "B'C"] and lex.lm is lm
    # the labels cannot spell <unk>, <s>, </s>: the model's trie is the lexicon's, whole-word marks included
    assert lex.shares_trie_with_lm(english_labels, 0)
    assert not Lexicon(['A', 'AB']).shares_trie_with_lm(english_labels, 0)
    odd = ['_', 'A', 'B', 'C', "'", ' ', '<', 's', '>']          # ... these can spell <s>
    assert not lex.shares_trie_with_lm(odd, 0)
    mine, theirs = lex.spelling_trie(english_labels, 0), lm.spelling_trie(english_labels, 0)
    assert np.array_equal(mine[0], theirs[0]) and np.array_equal(mine[1], theirs[1])
    assert [lex.words[i] for i in mine[2] if i >= 0] == [lm.words[i] for i in theirs[2] if i >= 0]


# ------------------------------------------------------------------------------------------ flat trie against the definition
WORDS7 = ['a', 'ab', 'abba', 'ba', 'cab', 'bcc', 'c']


def _legal_by_definition(words, s, end_char):
    """the module docstring's definition, restated with startswith (not Lexicon's prefix set)"""
    parts = s.replace(end_char, ' ').split(' ')
    closed = all(p == '' or p in words for p in parts[:-1])
    return closed and any(w.startswith(parts[-1]) for w in words + ['']), parts[-1] == '' or parts[-1] in words


def _device_rule(keys, vals, word, canon, seps, s):
    """the kernel's walk over the flat tables: (legal, complete) of the label string s"""
    table = dict(zip(keys.tolist(), vals.tolist()))
    node = 0
    for ch in s:
        c = canon[ch]
        if c in seps:
            if not (node == 0 or word[node] >= 0):
                return False, False
            node = 0
        else:
            node = table.get((node << 8) | c, -1)
            if node < 0:
                return False, False
    return True, bool(node == 0 or word[node] >= 0)


def test_flat_trie_matches_definition():
    labels = ['_', 'a', 'b', 'c', ' ', '>', 'b']                 # five symbols, and a duplicate label
    lex = Lexicon(WORDS7)
    keys, vals, word = lex.spelling_trie(labels, 0)
    assert lex.stats['unspellable'] == 0
    canon = {ch: labels.index(ch) for ch in labels}
    seps = {canon[' '], canon['>']}
    n = legal = 0
    for length in range(7):
        for tup in itertools.product('abc >', repeat=length):
            s = ''.join(tup)
            want = _legal_by_definition(WORDS7, s, '>')
            assert (lex.allows(s), lex.complete(s)) == want, s
            got = _device_rule(keys, vals, word, canon, seps, s)
            assert got[0] == want[0] and (not want[0] or got[1] == want[1]), (s, got, want)
            n += 1
            legal += want[0]
            if want[0]:                                          # legal strings are prefix-closed
                assert lex.allows(s[:-1])
    assert n == sum(5 ** i for i in range(7)) and 0 < legal < n
    assert lex.allows('abba ab  c>') and lex.complete('abba ab') and not lex.complete('abb') and lex.allows('abb')
    assert not lex.allows('abb ') and not lex.allows('abc') and lex.allows('  a') and lex.allows('')


# --------------------------------------------------------------------------------------- host recursion against brute force
BF_LABELS = ['_', 'a', 'b', 'c', ' ']
BF_T = 5


def _collapse(path):
    out, prev = [], 0
    for l in path:
        if l != prev and l != 0:
            out.append(BF_LABELS[l])
        prev = l
    return ''.join(out)


_BF_PATHS = list(itertools.product(range(5), repeat=BF_T))
_BF_STRINGS = [_collapse(p) for p in _BF_PATHS]


def _exact_masses(p):
    """float64 mass of every collapsed string: the sum over all 5^5 alignments"""
    mass = {}
    for path, s in zip(_BF_PATHS, _BF_STRINGS):
        mass[s] = mass.get(s, 0.0) + float(np.prod([p[t, l] for t, l in enumerate(path)]))
    return mass


@pytest.mark.parametrize('seed', range(20))
def test_host_oracle_against_brute_force(seed):
    lex = Lexicon(WORDS7)
    p = np.random.default_rng(seed).dirichlet(np.ones(5), size=BF_T)
    mass = _exact_masses(p)
    k = len(mass)                                                # nothing ever falls off the beam
    for complete_only in (True, False):
        keep = [s for s in mass if lex.allows(s) and (lex.complete(s) or not complete_only)]
        want = max(keep, key=lambda s: mass[s])
        got, w = prefix_beam_search(p, BF_LABELS, lm=None, k=k, beta=0, prune=0, return_weights=True, lexicon=lex,
                                    complete_only=complete_only)
        assert got == want, (got, want)
        assert abs(w - mass[want]) <= 1e-12 * mass[want], (w, mass[want])
    # (the unconstrained search finds the exact masses the same way: the enumeration is a fair oracle)
    got, w = prefix_beam_search(p, BF_LABELS, lm=None, k=k, beta=0, prune=0, return_weights=True)
    assert got == max(mass, key=lambda s: mass[s]) and abs(w - mass[got]) <= 1e-12 * mass[got]


def test_constraint_changes_a_decode():
    """some seed's unconstrained best is illegal, so the tests above are not vacuous"""
    lex = Lexicon(WORDS7)
    changed = 0
    for seed in range(20):
        p = np.random.default_rng(seed).dirichlet(np.ones(5), size=BF_T)
        changed += not lex.allows(prefix_beam_search(p, BF_LABELS, k=400, beta=0, prune=0))
    assert changed >= 3, changed


def test_repeat_branch_keeps_mass_of_the_prefix():
    """'abb' is legal, 'abbb' is not: the repeated b still feeds 'abb' itself (k = 1: everything else falls off)"""
    labels = ['_', 'a', 'b', ' ']
    lex = Lexicon(['abba'])
    p = np.array([[0.1, 0.8, 0.05, 0.05], [0.1, 0.1, 0.7, 0.1], [0.7, 0.1, 0.1, 0.1], [0.1, 0.1, 0.7, 0.1],
                  [0.1, 0.1, 0.7, 0.1], [0.1, 0.7, 0.1, 0.1]])
    for k in (1, 3, 50):
        got, w = prefix_beam_search(p, labels, k=k, beta=0, prune=0, return_weights=True, lexicon=lex)
        assert got == 'abba'
    # exact mass of 'abba' over all alignments
    mass = 0.0
    for path in itertools.product(range(4), repeat=6):
        out, prev = [], 0
        for l in path:
            if l != prev and l != 0:
                out.append(labels[l])
            prev = l
        if ''.join(out) == 'abba':
            mass += float(np.prod([p[t, l] for t, l in enumerate(path)]))
    assert abs(w - mass) <= 1e-12 * mass


# -------------------------------------------------------------------------------------------------------------------- no-op
def _asr_sample():
    s = np.zeros((10, len(english_labels)))
    s[0, 2] = 0.5
    s[1, 20] = 0.5
    s[2, 19] = 0.5
    s[3:, 0] = 0.5
    return s


def _every_string(letters, n):
    return [''.join(t) for i in range(1, n + 1) for t in itertools.product(letters, repeat=i)]


def test_no_lexicon_and_all_words_lexicon_change_nothing():
    def the_lm(s):
        return 0.5 if s == 'A' else 1
    ab = np.array([[0.8, 0.2, 0, 0], [0.6, 0.4, 0, 0]])
    width = np.array([[0.8, 0.2, 0], [0.7, 0.3, 0], [0.6, 0.4, 0], [0.0, 0.0, 1]])
    cases = [  # (posteriors, labels, keywords, the known answer of tests/test_beam_search.py, letters that pass the prune)
        (_asr_sample(), english_labels, dict(), 'ASR', 'ASR'),
        (ab, ['_', 'A', 'B', ' '], dict(blank_index=0, return_weights=True), ('A', 0.52), 'A'),
        (width, ['_', 'A', ' '], dict(lm=the_lm, k=25, alpha=1, beta=0), ' ', 'A'),
        (width, ['_', 'A', ' '], dict(lm=the_lm, k=1, alpha=1, beta=0), 'A ', 'A'),
        (width, ['_', 'A', ' '], dict(lm=the_lm, k=25, alpha=1, beta=0, return_weights=True), None, 'A'),
    ]
    for p, labels, kw, known, letters in cases:
        plain = prefix_beam_search(p, labels, **kw)
        assert known is None or plain == known
        assert prefix_beam_search(p, labels, lexicon=None, **kw) == plain
        everything = Lexicon(_every_string(letters, 4))
        assert prefix_beam_search(p, labels, lexicon=everything, complete_only=False, **kw) == plain


# ------------------------------------------------------------------------------------------------------------------- config
def test_command_line_rules():
    from wav2letter_pytorch_amd import test as T
    base = ['model_path=a.ckpt', 'data.test_manifest=m.csv']
    cfg = T.build_config(base + ['decoder=beam', 'lexicon_path=words.txt'])
    name, kw = T.decoder_spec(cfg, True)
    assert name == 'GPUPrefixBeamSearchDecoder' and kw['lexicon'] == 'words.txt' and kw['lm_path'] is None
    cfg = T.build_config(base + ['decoder=beam_lm', 'lm_path=lm.arpa', 'lexicon_path=words.txt', 'word_times=true'])
    name, kw = T.decoder_spec(cfg, True)
    assert name == 'GPUPrefixBeamSearchLMDecoder' and kw['lexicon'] == 'words.txt' and kw['lm_path'] == 'lm.arpa'
    assert cfg.word_times
    cfg = T.build_config(base + ['decoder=beam_lm', 'lm_path=lm.arpa', 'lexicon_from_lm=true'])
    assert T.decoder_spec(cfg, False)[1]['lexicon'] == 'lm'
    for dec in (['decoder=beam'], ['decoder=beam_lm', 'lm_path=lm.arpa']):        # no lexicon: the decoders' defaults
        assert 'lexicon' not in T.decoder_spec(T.build_config(base + dec), True)[1]
    with pytest.raises(SystemExit, match='both'):
        T.build_config(base + ['decoder=beam_lm', 'lm_path=lm.arpa', 'lexicon_from_lm=true', 'lexicon_path=words.txt'])
    with pytest.raises(SystemExit, match='lexicon_from_lm'):
        T.build_config(base + ['decoder=beam', 'lexicon_from_lm=true'])
    with pytest.raises(SystemExit, match='lexicon_path'):
        T.build_config(base + ['decoder=greedy', 'lexicon_path=words.txt'])
    with pytest.raises(SystemExit, match='lexicon_path'):
        T.build_config(base + ['lexicon_path=words.txt'])
    with pytest.raises(SystemExit, match='lexicon_from_lm'):
        T.build_config(base + ['lexicon_from_lm=true'])
    asg = base + ['model.criterion=asg']
    with pytest.raises(SystemExit, match='not built for ASG'):
        T.build_config(asg + ['decoder=asg_beam', 'lexicon_path=words.txt'])
    with pytest.raises(SystemExit, match='not built for ASG'):
        T.build_config(asg + ['decoder=asg_beam_lm', 'lm_path=lm.arpa', 'lexicon_from_lm=true'])


def test_decoder_constructors(tmp_path):
    from wav2letter_pytorch_amd.beam_search import GPUPrefixBeamSearchDecoder, GPUPrefixBeamSearchLMDecoder
    (tmp_path / 'm.arpa').write_text(SMALL_ARPA)
    (tmp_path / 'w.txt').write_text('A\nAB\n')
    d = GPUPrefixBeamSearchDecoder(None, english_labels, lexicon=str(tmp_path / 'w.txt'))
    assert d.lexicon.words == ['A', 'AB']
    assert GPUPrefixBeamSearchDecoder(None, english_labels).lexicon is None
    with pytest.raises(ValueError, match="'lm'"):
        GPUPrefixBeamSearchDecoder(None, english_labels, lexicon='lm')
    d = GPUPrefixBeamSearchLMDecoder(str(tmp_path / 'm.arpa'), english_labels, lexicon='lm')
    assert d.lexicon.words == ['A', 'AB', "B'C"] and d.lexicon.lm is d.lm
    lex = Lexicon(['A'])
    assert GPUPrefixBeamSearchLMDecoder(str(tmp_path / 'm.arpa'), english_labels, lexicon=lex).lexicon is lex
    with pytest.raises(ValueError, match="'lm'"):
        GPUPrefixBeamSearchLMDecoder(None, english_labels, lexicon='lm')
