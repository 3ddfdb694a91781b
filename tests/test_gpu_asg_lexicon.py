"""The ASG beam search with a lexicon and with hotwords (w2l_asg_beam_search_tables, all eight LM / lexicon / hotword
combinations) against the host restatement ``asg_prefix_beam_search(..., lexicon=, hotwords=)`` on the float64 widening of the
same scores: n-best strings, encoded hypotheses and order identical, scores within 1e-9 * max(1, |ref|) -- the bound of
tests/test_gpu_asg_beam.py for this fp64 arithmetic.

Scores are float32 log-softmax rows.  Three of the four utterances open with a scripted passage (A L r ' ', A B r A ' ',
B E D ' ': doubled letters are reached through the repeat label) and go on as bursts of a few letters, the repeat label or the
space with a rival boosted almost as much; the fourth spells only X, Y, Z, which no word holds.  No case is skipped for a
near-tie: the seeds below produce none (two candidates whose keys differ by less than the bound and straddle a beam edge would
show as a string mismatch)."""
import ctypes as C
import functools
import gc
import itertools

import numpy as np
import pytest
import torch

from asg_beam_refs import gen_arpa, log_softmax_scores, transitions
from asg_lexicon_refs import DEAD_K, DEAD_LABELS, DEAD_PRUNE, DEAD_WORDS, dead_beam_case, write_arpa
from wav2letter_pytorch_amd._lib import LexTables, lib, ptr, stream_ptr
from wav2letter_pytorch_amd.asg_beam import (ASGBeamSearchDecoder, ASGBeamSearchLMDecoder, _label_info, _search_device,
                                             _transitions_on, asg_beam_search_gpu, asg_forced_align, asg_prefix_beam_search)
from wav2letter_pytorch_amd.data.label_sets import english_labels
from wav2letter_pytorch_amd.lexicon import Lexicon

pytestmark = pytest.mark.gpu

LABELS = list(english_labels)                                   # '_' (the repeat label), "'", A .. Z, ' '
REP, SPACE = 0, LABELS.index(' ')
WORDS = ['A', 'AB', 'ABBA', 'ALL', 'BE', 'BED', 'CAB', "D'C", 'DEB', 'EB', 'C', 'LEAD', 'DÉJÀ']     # (the last: unspellable)
LM_WORDS = ['A', 'AB', 'ABBA', 'ALL', 'BE', 'BED', 'CAD', 'DEB', 'ELL', 'C', "E'D"]     # not the lexicon: some in, some out
HOTWORDS = ['ABBA', 'BED', 'DÉJÀ']
N = 4
SIZES = {24: [24, 17, 24, 24], 40: [40, 40, 29, 40]}
SCRIPT = ('AL_ ', 'AB_A ', 'BED ')
ALPHA = 0.5


@functools.lru_cache(maxsize=None)
def _lexicon():
    return Lexicon(WORDS)


@functools.lru_cache(maxsize=None)
def _hotwords():
    return Lexicon(HOTWORDS)


@functools.lru_cache(maxsize=None)
def _g():
    g = transitions(31, len(LABELS), scale=0.3)
    assert np.all(g != 0)
    return g


@functools.lru_cache(maxsize=None)
def _scores(t, seed=0):
    """float32 [4, t, 29]; shared by the tests, never written"""
    rng = np.random.default_rng(1000 * t + seed)
    a = len(LABELS)
    cand = [LABELS.index(c) for c in "ABCDEL'"] + [LABELS.index('A'), LABELS.index('B')]
    logits = rng.standard_normal((N, t, a))
    for u in range(N - 1):
        f, last = len(SCRIPT[u]), SPACE
        for j, ch in enumerate(SCRIPT[u]):
            logits[u, j, LABELS.index(ch)] += 9.0
        while f < t:
            if last not in (REP, SPACE) and rng.random() < 0.3:
                c = REP
            else:
                c = SPACE if rng.random() < 0.3 else cand[rng.integers(len(cand))]
            burst = int(rng.integers(1, 3))
            b = rng.uniform(3.0, 6.0)
            logits[u, f:f + burst, c] += b
            logits[u, f:f + burst, cand[rng.integers(len(cand))]] += b - rng.uniform(0, 1.5)
            f += burst
            last = c
    junk = [LABELS.index(c) for c in 'XYZ']                      # the last utterance: X, Y, Z, every other label 20 nats down
    logits[N - 1] -= 20.0
    logits[N - 1, :, junk] += 20.0
    for f in range(0, t, 3):
        logits[N - 1, f, junk[(f // 3) % 3]] += rng.uniform(3.0, 5.0)
    z = logits - logits.max(-1, keepdims=True)
    return (z - np.log(np.exp(z).sum(-1, keepdims=True))).astype(np.float32)


@pytest.fixture(scope='module')
def models(tmp_path_factory):
    d = tmp_path_factory.mktemp('asg_lex_lm')
    lms = dict(bigram=write_arpa(d / 'b.arpa', LM_WORDS, 2, 1), trigram=write_arpa(d / 't.arpa', WORDS[:-1], 3, 2))
    yield dict(lms, dir=d)
    # The models and the lexica made from them refer to each other (lm._lexicon.lm is lm) and own device tables: the cycles
    # are cut here and what this module leaves behind is collected at its end (_release_at_module_end), by the thread that
    # runs the tests and not by whichever thread a later test's collection happens to run on
    for lm in lms.values():
        for attr in ('_weigh', '_host_lex', '_lexicon'):
            lm.__dict__.pop(attr, None)


@pytest.fixture(scope='module', autouse=True)
def _release_at_module_end():
    yield
    _HOST.clear()
    for cached in (_lexicon, _hotwords, _g, _scores):
        cached.cache_clear()
    torch.cuda.synchronize()
    gc.collect()


def _weigh(lm):
    if lm is None:
        return None
    if not hasattr(lm, '_weigh'):
        lm._weigh = functools.lru_cache(maxsize=None)(lambda s: 10 ** lm.score(s))
    return lm._weigh


def _host_lexicon(lexicon, lm):
    if isinstance(lexicon, str):                                 # 'lm': the host's lexicon is the model's vocabulary
        if not hasattr(lm, '_host_lex'):
            lm._host_lex = Lexicon.from_lm(lm)
        return lm._host_lex
    return lexicon


_HOST = {}


def _host(x, g, labels, key, **kw):
    """asg_prefix_beam_search on the float64 widening of x, computed once per argument set"""
    if key not in _HOST:
        got = asg_prefix_beam_search(x.astype(np.float64), g.astype(np.float64), labels, return_weights=True,
                                     return_encoded=True, **kw)
        _HOST[key] = got if kw['nbest'] > 1 else [got]
    return _HOST[key]


def _close(got, ref):
    return abs(got - ref) <= 1e-9 * max(1.0, abs(ref))


def _check_rows(row, ref, lex, complete_only, where):
    assert [(s, e) for s, _, e in row] == [(s, e) for s, _, e in ref], (where, row[:3], ref[:3])
    for (_, w, e), (_, wr, _) in zip(row, ref):
        assert _close(w, wr), (where, e, w, wr)
    if lex is not None:
        for s, _, _ in row:
            assert lex.allows(s, end_char=''), (where, s)
        if complete_only and any(lex.complete(s, end_char='') for s, _, _ in row):
            assert all(lex.complete(s, end_char='') and all(wd in lex for wd in s.split()) for s, _, _ in row), (where, row)


def _compare(t, k, beta, prune, lm=None, lexicon=None, complete_only=True, hotwords=None, gamma=1.0, alpha=ALPHA):
    """device n-best lists of the four utterances against the host's -> the device lists"""
    x, g = _scores(t), _g()
    got = asg_beam_search_gpu(x, g, LABELS, k=k, beta=beta, prune=prune, sizes=SIZES[t], nbest=k, return_weights=True,
                              return_encoded=True, lm=lm, alpha=alpha, lexicon=lexicon, complete_only=complete_only,
                              hotwords=hotwords, hotword_weight=gamma)
    rows = [row if k > 1 else [row] for row in got]
    lex = _host_lexicon(lexicon, lm)
    for u in range(N):
        key = (t, u, k, beta, prune, id(lm), alpha, id(lex), complete_only, id(hotwords), gamma)
        ref = _host(x[u, :SIZES[t][u]], g, LABELS, key, k=k, beta=beta, prune=prune, nbest=k, lm=_weigh(lm), alpha=alpha,
                    lexicon=lex, complete_only=complete_only, hotwords=hotwords, hotword_weight=gamma)
        _check_rows(rows[u], ref, None if lex is None else lex.spellable(LABELS, REP), complete_only, (t, k, u))
    return rows


CASES = list(itertools.product((24, 40), (1, 3, 8, 32), (0, 5), (1e-3, 0)))


def test_the_unconstrained_decode_leaves_the_lexicon():
    """the premise of every comparison below: without the constraint every decode holds a word that is not in the lexicon"""
    lex = _lexicon()
    for t in (24, 40):
        plain = asg_beam_search_gpu(_scores(t), _g(), LABELS, k=8, sizes=SIZES[t])
        outside = [any(w not in lex for w in s.split()) for s in plain]
        assert all(outside), plain
        assert set(plain[N - 1]) <= set('XYZ')


@pytest.mark.parametrize('t,k,beta,prune', CASES)
def test_lexicon_only(t, k, beta, prune):
    lex = _lexicon()
    on = _compare(t, k, beta, prune, lexicon=lex)
    off = _compare(t, k, beta, prune, lexicon=lex, complete_only=False)
    assert lex.stats['unspellable'] == 1
    for a, b in zip(on, off):                                    # the filter drops members, it does not change them
        assert a == ([row for row in b if lex.complete(row[0], end_char='')] or b)


def test_a_doubled_letter_word_is_reached_through_the_repeat_label():
    a_, b_, l_ = (LABELS.index(c) for c in 'ABL')
    rows = _compare(24, 8, 5, 1e-3, lexicon=_lexicon())
    text, _, e = rows[0][0]
    assert text.split()[0] == 'ALL' and e[:3] == (a_, l_, REP)
    text, _, e = rows[1][0]
    assert text.split()[0] == 'ABBA' and e[:4] == (a_, b_, REP, a_)


@pytest.mark.parametrize('t,k,beta,prune', CASES)
def test_lexicon_with_bigram(models, t, k, beta, prune):
    """the lexicon is a separate list: some of its words are <unk> to the model, some of the model's words are banned"""
    for complete_only in (True, False):
        _compare(t, k, beta, prune, lm=models['bigram'], lexicon=_lexicon(), complete_only=complete_only)


@pytest.mark.parametrize('t,k,beta,prune', CASES)
def test_lexicon_from_lm(models, t, k, beta, prune):
    """lexicon='lm': the model's own trie (order 3), shared on the device"""
    lm = models['trigram']
    for complete_only in (True, False):
        _compare(t, k, beta, prune, lm=lm, lexicon='lm', complete_only=complete_only, alpha=0.7)
    assert lm._lexicon.to_device(LABELS, REP, 'cuda').shared


@pytest.mark.parametrize('with_lm,with_lex', [(False, False), (False, True), (True, False), (True, True)])
@pytest.mark.parametrize('t,k,beta,prune', CASES)
def test_hotwords_in_the_four_combinations(models, t, k, beta, prune, with_lm, with_lex):
    hot = _hotwords()
    kw = dict(lm=models['bigram'] if with_lm else None, lexicon=_lexicon() if with_lex else None)
    _compare(t, k, beta, prune, hotwords=hot, gamma=0.7, **kw)
    if k <= 3:                                                   # a penalty instead of a bonus, and the unfiltered beam
        _compare(t, k, beta, prune, hotwords=hot, gamma=-0.5, complete_only=False, **kw)
    assert hot.stats['unspellable'] == 1


def test_hotwords_change_a_decode():
    """... so that the comparisons above do not pass on a boost that never matters"""
    x, g = _scores(40), _g()
    plain = asg_beam_search_gpu(x, g, LABELS, k=8, sizes=SIZES[40], lexicon=_lexicon())
    boosted = asg_beam_search_gpu(x, g, LABELS, k=8, sizes=SIZES[40], lexicon=_lexicon(), hotwords=HOTWORDS, hotword_weight=2.0)
    assert plain != boosted
    assert sum(w in HOTWORDS for s in boosted for w in s.split()) > sum(w in HOTWORDS for s in plain for w in s.split())


# ------------------------------------------------------------------------------------------------------- participation rule
def test_the_beam_does_not_die_under_a_lexicon():
    x, g = dead_beam_case()
    lex = Lexicon(DEAD_WORDS)
    kw = dict(k=DEAD_K, prune=DEAD_PRUNE, beta=0, return_weights=True, return_encoded=True)
    ref = asg_prefix_beam_search(x.astype(np.float64), g.astype(np.float64), DEAD_LABELS, lexicon=lex, **kw)
    got = asg_beam_search_gpu(x, g, DEAD_LABELS, lexicon=lex, **kw)
    assert got[0] == ref[0] == 'AL' and got[2] == ref[2] and _close(got[1], ref[1])
    # two frames: the member that could neither stay nor extend by the unamended rule is still there
    got = asg_beam_search_gpu(x[:2], g, DEAD_LABELS, lexicon=lex, **kw)
    ref = asg_prefix_beam_search(x[:2].astype(np.float64), g.astype(np.float64), DEAD_LABELS, lexicon=lex, **kw)
    assert got[0] == ref[0] == 'A' and got[2] == ref[2] == (2,) and _close(got[1], ref[1])
    # without a lexicon, hotwords or not, the rule is the old one
    for extra in (dict(), dict(hotwords=DEAD_WORDS)):
        assert asg_beam_search_gpu(x, g, DEAD_LABELS, **kw, **extra)[0] == 'A L'


# ------------------------------------------------------------------------------------------------------------ byte equality
def _raw(x, g, sz, k, lm=None, **kw):
    return _search_device(x, g, sz, LABELS, REP, k, 5.0, 1e-3, lm, ALPHA, False, **kw)


def _same_bytes(a, b):
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()         # scores, lengths
    for u, r in zip(*np.nonzero(a[1] >= 0)):
        assert a[2][u, r, :a[1][u, r]].tobytes() == b[2][u, r, :a[1][u, r]].tobytes()
    if a[3] is not None:
        assert a[3].tobytes() == b[3].tobytes()


def test_weight_zero_is_byte_equal_to_no_hotwords(models):
    x = torch.from_numpy(_scores(40)).cuda()
    g = _transitions_on(_g(), len(LABELS), x.device)
    sz = torch.tensor(SIZES[40], dtype=torch.int32, device=x.device)
    for kw in (dict(), dict(lexicon=_lexicon()), dict(lm=models['bigram']), dict(lm=models['bigram'], lexicon=_lexicon())):
        for k in (3, 32):
            _same_bytes(_raw(x, g, sz, k, **kw), _raw(x, g, sz, k, hotwords=_hotwords(), hotword_weight=0.0, **kw))


def _direct(symbol, x, g, k, lm, order, tables, fill=0x5a):
    """one call of a search symbol on its own workspace and an ``out`` pre-filled with ``fill`` -> the whole buffer's bytes"""
    n, t, a = x.shape
    info = _label_info(LABELS, True)
    ws_bytes = int(lib.w2l_asg_beam_search_workspace_bytes(n, t, a, k, order))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=x.device)
    out = torch.full((12 * n * k + 4 * n + 4 * n * k * t + (4 * n * k if lm is not None else 0),), fill, dtype=torch.uint8,
                     device=x.device)
    head = (ptr(x), ptr(g), None, n, t, a, info.ctypes.data_as(C.c_void_p), REP, SPACE, k, ALPHA, 5.0, 1e-3, lm, order)
    tail = (ptr(ws), ws_bytes, ptr(out), stream_ptr())
    assert getattr(lib, symbol)(*head, *tables, *tail) == 0, lib.w2l_last_error()
    return out.cpu().numpy().tobytes()


def test_null_tables_are_the_older_symbol_byte_for_byte(models):
    x = torch.from_numpy(_scores(24)).cuda()
    g = _transitions_on(_g(), len(LABELS), x.device)
    lm = models['bigram']
    dev_lm = lm.to_device(LABELS, REP, x.device)
    dev_lex = _lexicon().to_device(LABELS, REP, x.device)
    dev_hot = _hotwords().to_device(LABELS, REP, x.device)
    for k in (4, 64):
        for lm_ref, order in ((None, 0), (dev_lm.desc_ref, lm.order)):
            before = _direct('w2l_asg_beam_search', x, g, k, lm_ref, order, ())
            assert _direct('w2l_asg_beam_search_tables', x, g, k, lm_ref, order, (None, 1, None, 0.0)) == before
            assert _direct('w2l_asg_beam_search_tables', x, g, k, lm_ref, order, (None, 0, None, float('nan'))) == before
            changed = _direct('w2l_asg_beam_search_tables', x, g, k, lm_ref, order, (dev_lex.desc_ref, 1, dev_hot.desc_ref, 0.7))
            assert changed != before
            assert _direct('w2l_asg_beam_search', x, g, k, lm_ref, order, ()) == before       # ... and after a tables call


# -------------------------------------------------------------------------------------------------------------- LDS limit
def test_lds_limit_64_labels_64_slots_all_tables(tmp_path):
    """k = 64 with A = 64 and the three tables: the largest static + dynamic LDS any instantiation asks for"""
    labels = ['_'] + [chr(0x100 + i) for i in range(62)] + [' ']
    letters = ''.join(labels[1:6])
    lm = gen_arpa(tmp_path / 'm.arpa', 6, 2, letters=letters)
    rng = np.random.default_rng(12)
    words = sorted({''.join(labels[i] for i in rng.integers(1, 63, size=rng.integers(1, 4))) for _ in range(400)}
                   | set([w for w in lm.words if w not in ('<unk>', '<s>', '</s>')][:37]))
    lex, hot = Lexicon(words), Lexicon(words[::7])
    x = log_softmax_scores(4, (8, 64), scale=2.0)
    g = transitions(9, 64)
    kw = dict(k=64, beta=5, prune=1e-4, nbest=64, return_weights=True, return_encoded=True, alpha=1.0)
    got = asg_beam_search_gpu(x, g, labels, lm=lm, lexicon=lex, hotwords=hot, hotword_weight=0.7, **kw)
    ref = asg_prefix_beam_search(x.astype(np.float64), g.astype(np.float64), labels, lm=_weigh(lm), lexicon=lex, hotwords=hot,
                                 hotword_weight=0.7, **kw)
    assert len(got) > 8
    _check_rows(got, ref, lex, True, 'k=64')


# ---------------------------------------------------------------------------------------------------------------- offsets
def test_return_offsets_under_a_lexicon(models):
    lex = _lexicon()
    for t, kw in ((24, dict(lexicon=lex)), (40, dict(lm=models['trigram'], alpha=0.7, lexicon='lm', hotwords=HOTWORDS))):
        x, g = _scores(t), _g()
        plain = asg_beam_search_gpu(x, g, LABELS, k=8, sizes=SIZES[t], return_encoded=True, **kw)
        rows, offsets = asg_beam_search_gpu(x, g, LABELS, k=8, sizes=SIZES[t], return_encoded=True, return_offsets=True, **kw)
        assert rows == plain
        res = asg_forced_align(x, g, [list(e) for _, _, e in rows], input_lengths=SIZES[t], labels=LABELS, encoded=True)
        for u, (text, _, e) in enumerate(rows):
            lead = 1 if e and e[0] == REP else 0
            off = offsets[u].tolist()
            assert offsets[u].dtype == torch.int32 and len(off) == len(text) == len(e) - lead, (u, text, e)
            assert all(a < b for a, b in zip(off, off[1:])) and (not off or 0 <= off[0] and off[-1] < SIZES[t][u])
            assert bool(res.feasible[u]) and off == res.starts[u, lead:len(e)].tolist(), (u, text)
        assert any(len(text) > 2 for text, _, _ in rows)
    dec = ASGBeamSearchDecoder(LABELS, transitions=_g(), k=8, lexicon=lex)
    xs = torch.from_numpy(_scores(24)).cuda()
    strings, offs = dec.decode(xs, torch.tensor(SIZES[24]), return_offsets=True)
    assert strings == asg_beam_search_gpu(xs, _g(), LABELS, k=8, sizes=SIZES[24], lexicon=lex)
    assert [len(o[0]) for o in offs] == [len(s) for s in strings]


# ------------------------------------------------------------------------------------------------------ the rejection matrix
def test_entry_point_errors(models):
    t, k = 24, 4
    x = torch.from_numpy(_scores(t)).cuda()
    g = _transitions_on(_g(), len(LABELS), x.device)
    lm = models['bigram']
    dev_lm = lm.to_device(LABELS, REP, 'cuda')
    good = _lexicon().to_device(LABELS, REP, 'cuda').desc
    info = _label_info(LABELS, True)
    tabbed = LABELS[:-3] + ['\t'] + LABELS[-2:]
    info_tab = _label_info(tabbed, True)
    ws_bytes = int(lib.w2l_asg_beam_search_workspace_bytes(N, t, len(LABELS), k, lm.order))
    small = int(lib.w2l_asg_beam_search_workspace_bytes(N, t, len(LABELS), k, 0))
    assert ws_bytes > small > 0
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device='cuda')
    out = torch.full((12 * N * k + 4 * N + 4 * N * k * t + 4 * N * k,), 0x5a, dtype=torch.uint8, device='cuda')

    def call(with_lm, lexicon=None, hotwords=None, weight=0.7, inf=info, sp=SPACE, size=ws_bytes):
        return lib.w2l_asg_beam_search_tables(ptr(x), ptr(g), None, N, t, len(LABELS), inf.ctypes.data_as(C.c_void_p), REP, sp, k,
                                              1.0, 5.0, 1e-3, dev_lm.desc_ref if with_lm else None, lm.order if with_lm else 0,
                                              lexicon, 1, hotwords, weight, ptr(ws), size, ptr(out), stream_ptr())

    def refused(rc, *words):
        msg = (lib.w2l_last_error() or b'').decode()
        assert rc != 0 and msg.startswith('asg_beam_search:'), (rc, msg)
        for w in words:
            assert w in msg, (w, msg)

    nodes = good.n_trie_nodes
    variants = dict(full=LexTables(good.trie_keys, good.trie_vals, good.trie_cap, good.trie_word, int(good.trie_cap // 2 + 2)),
                    odd_cap=LexTables(good.trie_keys, good.trie_vals, good.trie_cap - 1, good.trie_word, nodes),
                    no_keys=LexTables(None, good.trie_vals, good.trie_cap, good.trie_word, nodes),
                    no_word=LexTables(good.trie_keys, good.trie_vals, good.trie_cap, None, nodes))
    ok = C.byref(good)
    for with_lm in (False, True):
        for what, kw in (('lexicon', 'lexicon'), ('hotword', 'hotwords')):
            for kind, desc in variants.items():
                refused(call(with_lm, **{kw: C.byref(desc)}), what, 'NULL' if kind.startswith('no_') else 'capacity')
        for tables in (dict(lexicon=ok), dict(hotwords=ok), dict(lexicon=ok, hotwords=ok)):
            refused(call(with_lm, inf=info_tab, sp=-1, **tables), 'whitespace')
            refused(call(with_lm, sp=SPACE - 1, **tables), "other than ' '")
            refused(call(with_lm, sp=len(LABELS), **tables), 'space index')
        for weight in (float('inf'), float('-inf'), float('nan')):
            refused(call(with_lm, hotwords=ok, weight=weight), 'finite')
            refused(call(with_lm, lexicon=ok, hotwords=ok, weight=weight), 'finite')
        refused(call(with_lm, lexicon=ok, hotwords=ok, size=small - 1), 'workspace')
    torch.cuda.synchronize()
    assert bool((out == 0x5a).all())                             # nothing was launched
    for with_lm in (False, True):
        assert call(with_lm, lexicon=ok, hotwords=ok) == 0 and call(with_lm) == 0
    torch.cuda.synchronize()
    with pytest.raises(ValueError, match='whitespace'):
        asg_beam_search_gpu(_scores(t), None, tabbed, lexicon=_lexicon())
    with pytest.raises(TypeError):
        asg_beam_search_gpu(_scores(t), None, LABELS, lexicon=WORDS)
    with pytest.raises(ValueError, match="'lm'"):
        asg_beam_search_gpu(_scores(t), None, LABELS, lexicon='lm')
    with pytest.raises(ValueError, match='finite'):
        asg_beam_search_gpu(_scores(t), None, LABELS, hotwords=HOTWORDS, hotword_weight=float('nan'))


# ------------------------------------------------------------------------------------------------------------- end to end
def test_end_to_end_transcribe_and_evaluate(tmp_path):
    from asg_replay_worker import build_model, synthetic_batch
    from wav2letter_pytorch_amd.evaluate import evaluate
    model = build_model().cuda().eval()
    with torch.no_grad():
        model.criterion.transitions.copy_(torch.from_numpy(transitions(21, 29, scale=0.2)))
    lm = gen_arpa(tmp_path / 'm.arpa', 3, 2, letters=''.join(model.labels[2:7]))
    vocab = set(lm.words) - {'<unk>', '<s>', '</s>'}
    batch = synthetic_batch(model.labels)
    wave = (0.1 * np.random.default_rng(3).standard_normal(8000)).astype(np.float32)
    dec = ASGBeamSearchLMDecoder(str(tmp_path / 'm.arpa'), model.labels, transitions=model.criterion, k=4, lexicon='lm',
                                 hotwords=sorted(vocab)[:5], hotword_weight=0.5)
    hyps = model.transcribe([wave, wave[:6000]], decoder=dec)
    assert len(hyps) == 2 and all(isinstance(h, str) for h in hyps)
    metrics, records = evaluate(model, [batch], decoder=dec)
    assert len(records) == 4 and all(np.isfinite(metrics[key]) for key in ('test_loss', 'test_cer', 'test_wer'))
    texts = hyps + [r['hypothesis'] for r in records]
    assert all(w in vocab for s in texts for w in s.split()), texts
