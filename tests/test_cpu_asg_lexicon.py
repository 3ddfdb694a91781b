"""The lexicon constraint and hotword boosting of the ASG beam search without a GPU: the host oracle
(asg_beam.asg_prefix_beam_search) against a brute force over frame paths, decoded-character spelling, the hotword semantics,
the participation rule under a lexicon, the argument checks of w2l_asg_beam_search_tables (host pointers that a refused call
never reads through; on a GPU machine the matrix runs on device buffers in test_gpu_asg_lexicon.py) and the decoder classes'
constructors."""
import ctypes as C

import numpy as np
import pytest
import torch

from asg_beam_refs import brute_masses, gen_arpa, small_case
from asg_lexicon_refs import (DEAD_K, DEAD_LABELS, DEAD_PRUNE, DEAD_WORDS, LABELS4, brute_constrained_masses, dead_beam_case,
                              unamended_participants)
from wav2letter_pytorch_amd import asg_beam
from wav2letter_pytorch_amd._lib import EXPORTED_SYMBOLS, TRACE_NAMES, LexTables, LmTables, lib
from wav2letter_pytorch_amd.asg_beam import ASGBeamSearchDecoder, ASGBeamSearchLMDecoder, asg_prefix_beam_search
from wav2letter_pytorch_amd.data.label_sets import english_labels
from wav2letter_pytorch_amd.lexicon import Lexicon

ALL_K = 512          # 4 + 12 + 36 + 108 + 324 = 484 encoded hypotheses of up to 5 frames over 4 labels: nothing is pruned


def _search(x, g, **kw):
    kw.setdefault('k', ALL_K)
    kw.setdefault('beta', 0)
    kw.setdefault('prune', 0)
    return asg_prefix_beam_search(x, g, LABELS4, nbest=kw['k'], return_weights=True, return_encoded=True, **kw)


# ------------------------------------------------------------------------------------------------- oracle against brute force
@pytest.mark.parametrize('seed,t', [(0, 3), (1, 4), (2, 5), (3, 5)])
def test_oracle_equals_brute_force(seed, t):
    x, g = small_case(seed, a=4, t=t)
    lex = Lexicon(['A', 'AL', 'ALL', 'LA'])
    want = brute_constrained_masses(x, g, LABELS4, lex)
    free, _, _ = brute_masses(x, g)
    assert 0 < len(want) < len(free)                            # the constraint removes hypotheses ...
    assert all(want[e] == pytest.approx(free[e], abs=1e-12) for e in want)   # ... and legal strings are prefix-closed
    got = _search(x, g, lexicon=lex, complete_only=False)
    assert {e for _, _, e in got} == set(want)
    for text, w, e in got:
        assert lex.allows(text, end_char='')
        assert abs(w - want[e]) <= 1e-9 * max(1.0, abs(want[e])), (e, w, want[e])
    done = _search(x, g, lexicon=lex)
    assert done == [row for row in got if lex.complete(row[0], end_char='')]        # rank order, their own weights
    assert 0 < len(done) < len(got)


def test_complete_only_falls_back_to_the_whole_beam():
    x, g = small_case(4, a=4, t=2)
    lex = Lexicon(['ALLA'])
    x[:, :2] -= 50.0                                            # neither the repeat label nor the space
    got = _search(x, g, lexicon=lex, complete_only=False, k=2)
    assert [t for t, _, _ in got] == ['A', 'AL'] or [t for t, _, _ in got] == ['AL', 'A']
    assert _search(x, g, lexicon=lex, k=2) == got


# ------------------------------------------------------------------------------------------------------- decoded spelling
def _reachable(encoded, words):
    """whether the oracle, nothing pruned, keeps the hypothesis ``encoded`` on frames that spell it"""
    x = np.full((len(encoded), 4), -30.0)
    x[np.arange(len(encoded)), list(encoded)] = 0.0
    got = _search(x, None, lexicon=Lexicon(words), complete_only=False)
    return tuple(encoded) in {e for _, _, e in got}


def test_words_are_spelled_by_decoded_characters():
    r, sp, a, l = 0, 1, 2, 3
    words = ['ALL', 'A']
    assert _reachable((a, l, r), words)                         # A L r spells ALL
    assert not _reachable((a, l, a), words)                     # ALA
    assert not _reachable((a, r), words)                        # AA
    assert _reachable((r,), words) and _reachable((r, a), words)             # a leading r spells nothing
    assert _reachable((a, sp, r), words)                        # a second space
    assert _reachable((a, sp, r, a, l, r, sp), words)           # 'A  ALL '
    assert not _reachable((a, l, sp), words)                    # AL is no word
    # the best hypothesis on frames that read A L r: the text has the doubled letter
    x = np.full((3, 4), -30.0)
    x[[0, 1, 2], [a, l, r]] = 0.0
    assert asg_prefix_beam_search(x, None, LABELS4, k=4, lexicon=Lexicon(words), return_encoded=True)[::2] == ('ALL', (a, l, r))


# ------------------------------------------------------------------------------------------------------- hotword semantics
def test_hotword_weight_zero_is_the_unboosted_search():
    x, g = small_case(6, a=4, t=5)
    for kw in (dict(), dict(lexicon=Lexicon(['A', 'AL', 'LA', 'ALL']))):
        for k in (3, ALL_K):
            plain = _search(x, g, k=k, beta=2, prune=1e-3, **kw)
            assert _search(x, g, k=k, beta=2, prune=1e-3, hotwords=['LA'], hotword_weight=0.0, **kw) == plain    # identical keys


def test_hotwords_change_the_order_not_the_masses():
    x = np.full((2, 4), -9.0)
    x[0, 2:] = (-1.0, -1.1)
    x[1, 2:] = (-1.1, -1.0)
    plain = _search(x, None)
    assert plain[0][0] == 'AL'                                  # -2.0 against LA at -2.2
    hot = Lexicon(['LA'])
    boosted = _search(x, None, hotwords=hot, hotword_weight=1.0)
    assert boosted[0][0] == 'LA' and boosted[0][1] == pytest.approx(-2.2 + 2.0, abs=1e-9)
    mass = {e: w for _, w, e in plain}
    assert {e for _, _, e in boosted} == set(mass)
    for text, w, e in boosted:                                  # key = the same mass + weight * h
        assert w - 1.0 * hot.boost_chars(text, end_char='') == pytest.approx(mass[e], abs=1e-12)
    # the accepted forms, and a weight that is not finite
    assert _search(x, None, hotwords=['LA'], hotword_weight=1.0) == boosted
    with pytest.raises(ValueError, match='finite'):
        _search(x, None, hotwords=['LA'], hotword_weight=float('nan'))


# ------------------------------------------------------------------------------------------------------ participation rule
def test_the_beam_does_not_die_under_a_lexicon():
    x, g = dead_beam_case()
    lex = Lexicon(DEAD_WORDS)
    kw = dict(k=DEAD_K, prune=DEAD_PRUNE, beta=0, return_encoded=True)
    # the premise: after frame 0 the beam is ('A',); by the unamended rule frame 1 offers the space alone, the member cannot
    # stay and its one extension is illegal -- no candidate gets mass
    assert asg_prefix_beam_search(x[:1], g, DEAD_LABELS, lexicon=lex, **kw)[::2] == ('A', (2,))
    assert unamended_participants(x[1], DEAD_PRUNE) == [1]
    assert not lex.allows('A ', end_char='')
    # without a lexicon nothing changes: the unamended rule, and the illegal string wins
    assert asg_prefix_beam_search(x, g, DEAD_LABELS, **kw)[0] == 'A L'
    # with it the member stays through frame 1
    assert asg_prefix_beam_search(x[:2], g, DEAD_LABELS, lexicon=lex, **kw)[::2] == ('A', (2,))
    text, w, e = asg_prefix_beam_search(x, g, DEAD_LABELS, lexicon=lex, **kw)
    assert np.isfinite(w)
    assert (text, e) == ('AL', (2, 3)) and lex.allows(text, end_char='') and lex.complete(text, end_char='')
    # hotwords alone do not amend the rule
    assert asg_prefix_beam_search(x, g, DEAD_LABELS, hotwords=DEAD_WORDS, **kw)[0] == 'A L'


# ------------------------------------------------------------------------------------------------------- the C entry point
LABELS = list(english_labels)
N, T, K = 2, 24, 4


def test_the_symbol_is_registered():
    assert 'w2l_asg_beam_search_tables' in EXPORTED_SYMBOLS and hasattr(lib, 'w2l_asg_beam_search_tables')
    assert TRACE_NAMES['w2l_asg_beam_search_tables'] == TRACE_NAMES['w2l_asg_beam_search'] == 'asg_beam_search_kernel'
    assert lib.w2l_abi_version() == 2


class _Args:
    """host stand-ins for the buffers of a call, and descriptors that pass every check"""

    def __init__(self):
        self.buf = np.zeros(1 << 16, dtype=np.uint8)             # scores / workspace / out: never read by a refused call
        self.p = C.c_void_p(self.buf.ctypes.data)
        self.space = LABELS.index(' ')
        tabbed = LABELS[:-3] + ['\t'] + LABELS[-2:]
        self.info = asg_beam._label_info(LABELS, True)
        self.info_tab = asg_beam._label_info(tabbed, True)
        a = self.buf.ctypes.data
        self.lm = LmTables(a, a, a, a, 16, a, a, 16, a, 3, 3, 4)
        self.trie = LexTables(a, a, 16, a, 4)

    def trie_variants(self):
        g = self.trie
        return dict(full=LexTables(g.trie_keys, g.trie_vals, g.trie_cap, g.trie_word, int(g.trie_cap // 2 + 2)),
                    odd_cap=LexTables(g.trie_keys, g.trie_vals, g.trie_cap - 1, g.trie_word, g.n_trie_nodes),
                    no_keys=LexTables(None, g.trie_vals, g.trie_cap, g.trie_word, g.n_trie_nodes),
                    no_word=LexTables(g.trie_keys, g.trie_vals, g.trie_cap, None, g.n_trie_nodes))

    def call(self, info=None, space=None, lm=None, order=2, lexicon=None, hotwords=None, weight=0.7, k=K, a=None, repeat=0,
             x=True, ws_bytes=1 << 16):
        info = self.info if info is None else info
        return lib.w2l_asg_beam_search_tables(self.p if x else None, self.p, None, N, T, len(LABELS) if a is None else a,
                                              info.ctypes.data_as(C.c_void_p), repeat, self.space if space is None else space,
                                              k, 1.0, 5.0, 1e-3, lm, order, lexicon, 1, hotwords, weight, self.p, ws_bytes,
                                              self.p, None)


def _refused(rc, *words):
    msg = (lib.w2l_last_error() or b'').decode()
    assert rc != 0 and msg.startswith('asg_beam_search:'), (rc, msg)
    for w in words:
        assert w in msg, (w, msg)


@pytest.mark.skipif(torch.cuda.is_available(), reason='host pointers: test_gpu_asg_lexicon.py runs this matrix on device buffers')
def test_tables_entry_refuses_before_any_launch():
    s = _Args()
    lm, good = C.byref(s.lm), C.byref(s.trie)
    for with_lm in (None, lm):
        for what, kw in (('lexicon', 'lexicon'), ('hotword', 'hotwords')):
            other = 'hotwords' if kw == 'lexicon' else 'lexicon'
            for with_other in (None, good):
                for kind, desc in s.trie_variants().items():
                    words = ('NULL',) if kind.startswith('no_') else ('capacity',)
                    _refused(s.call(lm=with_lm, **{kw: C.byref(desc), other: with_other}), what, *words)
        for tables in (dict(lexicon=good), dict(hotwords=good), dict(lexicon=good, hotwords=good)):
            _refused(s.call(info=s.info_tab, space=-1, lm=with_lm, **tables), 'whitespace')       # a tab among the labels
            _refused(s.call(space=s.space - 1, lm=with_lm, **tables), "other than ' '")           # not the index of ' '
            _refused(s.call(space=len(LABELS), lm=with_lm, **tables), 'space index')
        for weight in (float('inf'), float('-inf'), float('nan')):
            for lexicon in (None, good):
                _refused(s.call(lm=with_lm, lexicon=lexicon, hotwords=good, weight=weight), 'finite')
    # the checks the older symbol makes, through this one, with and without tables
    _refused(s.call(lm=lm, order=7), 'order')
    for tables in (dict(), dict(lm=lm, lexicon=good, hotwords=good)):
        _refused(s.call(k=0, **tables), 'beam width')
        _refused(s.call(k=65, **tables), 'beam width')
        _refused(s.call(a=65, **tables), 'labels')
        _refused(s.call(repeat=len(LABELS), **tables), 'repeat_index')
        _refused(s.call(x=False, **tables), 'bad arguments')
    # a workspace below the query's answer: the tables add nothing to it
    small = lib.w2l_asg_beam_search_workspace_bytes(N, T, len(LABELS), K, 0)
    for tables, size in ((dict(), small - 1), (dict(lexicon=good, hotwords=good), small - 1), (dict(lm=lm, lexicon=good), small)):
        _refused(s.call(ws_bytes=size, **tables), 'workspace')


# ---------------------------------------------------------------------------------------------------------- the decoders
def test_decoder_constructors(tmp_path):
    lex = Lexicon(['ALL', 'ABBA', "D'C"])
    dec = ASGBeamSearchDecoder(english_labels, k=7, lexicon=lex, complete_only=False, hotwords=['ABBA', 'BE'], hotword_weight=0.5)
    assert dec.lexicon is lex and dec.complete_only is False and dec.hotword_weight == 0.5 and dec.k == 7
    assert isinstance(dec.hotwords, Lexicon) and dec.hotwords.words == ['ABBA', 'BE']
    plain = ASGBeamSearchDecoder(english_labels)
    assert plain.lexicon is None and plain.hotwords is None and plain.complete_only is True and plain.hotword_weight == 1.0
    words = tmp_path / 'words.txt'
    words.write_text('ALL A L L\nABBA A B B A\n')
    assert ASGBeamSearchDecoder(english_labels, lexicon=str(words), hotwords=str(words)).lexicon.words == ['ALL', 'ABBA']
    with pytest.raises(ValueError, match="'lm'"):
        ASGBeamSearchDecoder(english_labels, lexicon='lm')
    with pytest.raises(ValueError, match="'lm'"):
        ASGBeamSearchLMDecoder(None, english_labels, lexicon='lm')                # a falsy path: no model
    with pytest.raises(TypeError):
        ASGBeamSearchDecoder(english_labels, lexicon=['ALL'])
    with pytest.raises(ValueError, match='finite'):
        ASGBeamSearchDecoder(english_labels, hotwords=['ALL'], hotword_weight=float('inf'))
    with pytest.raises(ValueError):
        ASGBeamSearchDecoder(english_labels, hotwords=['two words'])
    with pytest.raises(ValueError, match='spelled'):
        ASGBeamSearchDecoder(english_labels, hotwords=['a_b'])                   # the repeat label's character spells nothing
    lm = gen_arpa(tmp_path / 'm.arpa', 3, 2)
    dlm = ASGBeamSearchLMDecoder(str(tmp_path / 'm.arpa'), english_labels, alpha=0.9, lexicon='lm', hotwords=lex,
                                 hotword_weight=-0.25)
    assert dlm.lexicon.lm is dlm.lm and set(dlm.lexicon.words) == set(lm.words) - {'<unk>', '<s>', '</s>'}
    assert dlm.hotwords is lex and dlm.hotword_weight == -0.25 and dlm.alpha == 0.9 and dlm.complete_only is True
    assert ASGBeamSearchLMDecoder(None, english_labels, lexicon=lex).lexicon is lex
