"""CTC keyword search without a GPU: the host model (keyword_search.keyword_scan_host / pick_hits_host) against the brute force
and the references of tests/kws_refs.py, the fp32 error bound the device tests use, the KeywordTable's packing, the argument
errors, the exported symbols -- and planted defects, each shown to be caught."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kws_refs as R  # noqa: E402

from wav2letter_pytorch_amd import keyword_search as KS  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NINF = float('-inf')

# (seed, T, keyword, share of -inf entries): S = 1, a doubled letter, T < 2 S - 1 frames short of the twins' blank, -inf entries
BRUTE_CASES = [(1, 40, [2, 4, 1], 0.0), (2, 23, [3], 0.0), (3, 31, [2, 2, 4], 0.0), (4, 3, [2, 2, 4], 0.0), (5, 2, [1, 2, 3], 0.0),
               (6, 29, [5, 1], 0.3), (7, 26, [1, 1], 0.25)]


@pytest.mark.parametrize('seed,T,kw,holes', BRUTE_CASES)
def test_scan_equals_brute_force(seed, T, kw, holes):
    lp = R.random_lp(seed, T, 6, holes).astype(np.float64)
    want_sc, want_st, unique = R.brute_force(lp, kw)
    sc, st = KS.keyword_scan_host(lp, kw)
    ref = R.scan_ref(lp, kw)
    finite = want_sc > NINF
    assert np.array_equal(sc > NINF, finite) and np.array_equal(ref['end_score'] > NINF, finite)
    assert np.abs(sc[finite] - want_sc[finite]).max(initial=0.0) <= 1e-9
    assert np.abs(ref['end_score'][finite] - want_sc[finite]).max(initial=0.0) <= 1e-9
    assert np.array_equal(st[unique], want_st[unique]) and np.array_equal(ref['end_start'][unique], want_st[unique])
    assert (st[~finite] == -1).all() and (sc <= 0).all()
    # the two restatements agree bit for bit, ties included
    assert np.array_equal(sc, ref['end_score']) and np.array_equal(st, ref['end_start'])
    if T < len(kw) + sum(a == b for a, b in zip(kw, kw[1:])):
        assert not finite.any()
    elif not holes:
        assert finite.any()


def test_past_the_length_and_the_input_checks():
    lp = R.random_lp(11, 12, 6)
    sc, st = KS.keyword_scan_host(lp, [2, 3], length=7)
    full, _ = KS.keyword_scan_host(lp[:7], [2, 3])
    assert np.array_equal(sc[:7], full) and (sc[7:] == NINF).all() and (st[7:] == -1).all()
    sc, st = KS.keyword_scan_host(lp, [2, 3], length=0)
    assert (sc == NINF).all() and (st == -1).all()
    bad = lp.copy()
    bad[4] = NINF
    for kw, x in (([], lp), ([0, 1], lp), ([6], lp), ([-1], lp), ([1] * 256, lp), ([1], bad)):
        with pytest.raises(ValueError):
            KS.keyword_scan_host(x, kw)


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_planted_occurrences_score_exactly_zero(dtype):
    lp = R.planted_lp(21, 32, 6, R.path_of(R.PLANTED_SPANS), dtype)
    sc, st = KS.keyword_scan_host(lp, R.PLANTED_KW, dtype=dtype)
    assert sc.dtype == dtype
    # 0 on every frame of the last character, the start exact; below 0 on the frame before and the frame after
    for (s, e), last in zip(R.PLANTED_SEGMENTS, ([11, 12, 13], [25, 26, 27])):
        assert last[-1] == e and (sc[last] == 0).all() and (st[last] == s).all() and sc[last[0] - 1] < 0 and sc[e + 1] < 0
    hits = KS.pick_hits_host(sc, st, -1.0 * len(R.PLANTED_KW), 8)
    assert [(h[0], h[1]) for h in hits] == R.PLANTED_SEGMENTS and all(h[2] == 0 for h in hits)
    assert hits == R.pick_ref(sc, st, -1.0 * len(R.PLANTED_KW), 8)


def test_pick_rule():
    sc = np.full(30, NINF)
    st = np.full(30, -1)
    # a plateau of zeros on frames 5..8 from start 2: the hit extends to the last of them
    sc[5:9], st[5:9] = 0.0, 2
    # a second, worse occurrence, and one that overlaps the first
    sc[15], st[15] = -0.5, 12
    sc[10], st[10] = -0.1, 8
    sc[20], st[20] = -2.0, 18
    assert KS.pick_hits_host(sc, st, -1.0, 8) == [(2, 8, 0.0), (12, 15, -0.5)]          # [8, 10] overlaps [2, 8]; -2 is under thr
    assert KS.pick_hits_host(sc, st, -2.0, 8) == [(2, 8, 0.0), (12, 15, -0.5), (18, 20, -2.0)]     # the threshold edge: >=
    assert KS.pick_hits_host(sc, st, np.nextafter(-2.0, 0), 8) == [(2, 8, 0.0), (12, 15, -0.5)]
    assert KS.pick_hits_host(sc, st, -2.0, 2) == [(2, 8, 0.0), (12, 15, -0.5)]           # truncation keeps the best
    assert KS.pick_hits_host(sc, st, -2.0, 1) == [(2, 8, 0.0)]
    # equal scores: the earlier start first, and of one start the later end
    sc2 = np.full(12, NINF)
    st2 = np.full(12, -1)
    sc2[[3, 4, 9]], st2[[3, 4, 9]] = -0.25, [1, 1, 6]
    assert KS.pick_hits_host(sc2, st2, -1.0, 1) == [(1, 4, -0.25)]
    assert KS.pick_hits_host(sc2, st2, -1.0, 8) == [(1, 4, -0.25), (6, 9, -0.25)]
    # a better, later hit suppresses an earlier overlapping one
    sc3 = np.full(12, NINF)
    st3 = np.full(12, -1)
    sc3[[5, 7]], st3[[5, 7]] = [-0.5, -0.2], [2, 4]
    assert KS.pick_hits_host(sc3, st3, -1.0, 8) == [(4, 7, pytest.approx(-0.2))]
    for curves in ((sc, st), (sc2, st2), (sc3, st3)):
        for thr in (-0.1, -1.0, -2.0):
            for mh in (1, 2, 8):
                assert KS.pick_hits_host(*curves, thr, mh) == R.pick_ref(*curves, thr, mh)
    g = np.random.default_rng(5)
    for _ in range(20):
        T = 60
        rs = -3.0 * g.random(T)
        rs[g.random(T) < 0.3] = NINF
        rs[g.random(T) < 0.2] = 0.0
        rst = np.maximum(0, np.arange(T) - g.integers(0, 6, T))
        rst[rs == NINF] = -1
        assert KS.pick_hits_host(rs, rst, -1.5, 5) == R.pick_ref(rs, rst, -1.5, 5)
    for mh in (0, 65):
        with pytest.raises(ValueError):
            KS.pick_hits_host(sc, st, -1.0, mh)


def _states_of(chunk):
    """(keyword, its lanes) of a packed chunk, in lane order"""
    out = {}
    for lane, m in enumerate(chunk['meta'].tolist()):
        if m >= 0:
            out.setdefault(m >> 4, []).append(lane)
    return out


def test_keyword_table_packing():
    g = np.random.default_rng(2)
    kws = [g.integers(1, 6, int(n)).tolist() for n in g.integers(1, 13, 40)]
    kws[7] = [2, 2, 4]
    table = KS.KeywordTable(kws)
    assert len(table) == 40 and len(table.chunks) == 1 and table.lengths.tolist() == [len(k) for k in kws]
    c = table.chunks[0]
    W = c['width']
    assert W == 64 and c['n_blocks'] >= 2 and len(c['labels']) == len(c['meta']) == c['n_blocks'] * W
    lanes = _states_of(c)
    assert sorted(lanes) == list(range(40))                              # every keyword, in order
    prev_last = -1
    for k, kw in enumerate(kws):
        ls = lanes[k]
        assert len(ls) == 2 * len(kw) - 1 and ls == list(range(ls[0], ls[0] + len(ls)))       # contiguous
        assert ls[0] // W == ls[-1] // W                                 # never split across blocks
        assert ls[0] > prev_last                                         # order preserved
        prev_last = ls[-1]
        assert c['block_kw'][ls[0] // W] <= k < c['block_kw'][ls[0] // W + 1]
        for i, lane in enumerate(ls):
            flags = int(c['meta'][lane]) & 15
            assert bool(flags & KS.FIRST) == (i == 0) and bool(flags & KS.LAST) == (i == len(ls) - 1)
            assert bool(flags & KS.LABEL) == (i % 2 == 0)
            if i % 2 == 0:
                assert c['labels'][lane] == kw[i // 2]
                assert bool(flags & KS.SKIP) == (i >= 2 and kw[i // 2] != kw[i // 2 - 1])
            else:
                assert not flags & KS.SKIP
    assert not KS.SKIP & int(c['meta'][lanes[7][2]])                     # the twins: no skip
    # greedy in the given order: a keyword opens a new block only when it does not fit the rest of the current one
    for b in range(c['n_blocks'] - 1):
        used = sum(len(lanes[k]) for k in range(c['block_kw'][b], c['block_kw'][b + 1]))
        assert used <= W and used + len(lanes[int(c['block_kw'][b + 1])]) > W
    assert c['block_kw'][0] == 0 and c['block_kw'][-1] == 40
    # widths as planned: the narrowest block that holds the longest keyword
    for s_max, want in ((1, 64), (32, 64), (33, 128), (64, 128), (65, 256), (128, 256), (129, 512), (255, 512)):
        t = KS.KeywordTable([[1] * 1, [1, 2] * (s_max // 2) + [1] * (s_max % 2)])
        assert t.chunks[0]['width'] == want == KS.plan_width(2 * s_max - 1), s_max
    one = KS.KeywordTable([[3] * 255])
    assert one.chunks[0]['width'] == 512 and one.chunks[0]['n_blocks'] == 1 and (one.chunks[0]['meta'] >= 0).sum() == 509
    assert KS.KeywordTable(kws, width=1024).chunks[0]['width'] == 1024
    with pytest.raises(ValueError):
        KS.KeywordTable([[3] * 40], width=64)
    # 4097 keywords: two chunks, the second with one keyword, indices local to the chunk
    many = KS.KeywordTable([[1 + i % 5, 1 + i % 3] for i in range(4097)])
    assert [(ch['k0'], ch['k1']) for ch in many.chunks] == [(0, 4096), (4096, 4097)]
    assert sorted(_states_of(many.chunks[0])) == list(range(4096)) and sorted(_states_of(many.chunks[1])) == [0]
    assert many.chunks[0]['n_blocks'] <= 4096
    # strings: a character maps to its first index
    labels = ['_', 'a', 'b', ' ', 'a']
    t = KS.KeywordTable(['ab a', 'b'], labels=labels)
    assert t.keywords == [(1, 2, 3, 1), (2,)] and t.texts == ['ab a', 'b']


def test_host_argument_errors():
    labels = ['_', 'a', 'b', ' ']
    for bad in ([''], ['ac'], ['a_'], ['a' * 256], [[]], [[1, 0]], [[4]], [[-1]], []):
        with pytest.raises(ValueError):
            KS.KeywordTable(bad, labels=labels)
    with pytest.raises(ValueError):
        KS.KeywordTable(['ab'])                                          # strings without labels
    x = np.zeros((1, 5, 4), dtype=np.float32)
    for kw in (dict(max_hits=0), dict(max_hits=65), dict(threshold=float('nan'))):
        with pytest.raises(ValueError):
            KS.ctc_keyword_search(x, ['ab'], labels=labels, **kw)
    for bad in ([''], ['ac'], ['a_'], ['a' * 256]):
        with pytest.raises(ValueError):
            KS.ctc_keyword_search(x, bad, labels=labels)
    with pytest.raises(ValueError):
        KS.ctc_keyword_search(x, [[1, 5]])                               # a label outside [0, A)
    with pytest.raises(ValueError):
        KS.ctc_keyword_search(x, [[1, 2]], input_lengths=[6])
    with pytest.raises(ValueError):
        KS.ctc_keyword_search(x, KS.KeywordTable([[1, 2]], blank=3), blank=0)
    with pytest.raises(ValueError):
        KS.ctc_keyword_search(np.zeros((1, 32769, 4), dtype=np.float32), [[1]])


def test_symbols_header_and_abi():
    from wav2letter_pytorch_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'w2l_hip.h')).read()
    assert re.search(r'\bint64_t w2l_ctc_kws_workspace_bytes\(', hdr) and re.search(r'\bint w2l_ctc_kws\(', hdr)
    assert 'w2l_kws_table_t' in hdr and 'w2l_kws_hit_t' in hdr
    for name in ('w2l_ctc_kws', 'w2l_ctc_kws_workspace_bytes'):
        assert name in _lib.EXPORTED_SYMBOLS and getattr(_lib.lib, name)
        assert _lib.lib.w2l_replay_op(name.encode()) == -1               # no replay entries
    assert _lib.lib.w2l_abi_version() == 2
    ws = _lib.lib.w2l_ctc_kws_workspace_bytes
    assert ws(32, 500, 256, 8) == 32 * 500 * 4 + 32 * 4
    for bad in ((0, 5, 1, 8), (1, 0, 1, 8), (1, 32769, 1, 8), (1, 5, 0, 8), (1, 5, 4097, 8), (1, 5, 1, 0), (1, 5, 1, 65)):
        assert ws(*bad) == -1, bad
    assert ws(1, 32768, 4096, 64) > 0
    assert KS.HIT_DTYPE.itemsize == 12


FP32_CASES = [(31, 40, 6, [2, 4, 1]), (32, 100, 29, [7, 7, 12, 3, 20]), (33, 300, 29, list(range(1, 29)) * 9 + [1, 2, 3]), (34, 17, 6, [3])]


@pytest.mark.parametrize('seed,T,A,kw', FP32_CASES)
def test_float32_scan_within_the_bound(seed, T, A, kw):
    lp = R.random_lp(seed, T, A, 0.1 if seed == 32 else 0.0)              # (fp32 values: both scans read the same numbers)
    ref = R.scan_ref(lp, kw)
    sc, st = KS.keyword_scan_host(lp, kw, dtype=np.float32)
    finite = ref['end_score'] > NINF
    assert np.array_equal(sc > NINF, finite)
    err = np.abs(sc[finite].astype(np.float64) - ref['end_score'][finite]).max(initial=0.0)
    bound = R.kws_bound(T, ref['P'])
    print(f'T={T} S={len(kw)}: fp32 error {err:.3e}, bound {bound:.3e} (P = {ref["P"]:.1f})')
    assert err <= bound
    assert finite.any()


@pytest.mark.parametrize('defect', R.DEFECTS)
def test_planted_defects_are_caught(defect):
    """each defect, planted in the reference scan, leaves the bound against the model or changes a hit"""
    caught = []
    # twins: without the blank between them a path of fewer frames spells the keyword
    lp = R.random_lp(41, 30, 6).astype(np.float64)
    kw = {'twin_skip': [2, 2, 4], 'enter_first': R.PLANTED_KW, 'no_b': [2, 4, 1], 'enter_blank': [2, 4, 1]}[defect]
    if defect == 'enter_first':
        lp = R.planted_lp(21, 32, 6, R.path_of(R.PLANTED_SPANS), np.float64)
    good_sc, good_st = KS.keyword_scan_host(lp, kw)
    bad = R.scan_ref(lp, kw, defect=defect)
    ok = R.scan_ref(lp, kw)
    assert np.array_equal(ok['end_score'], good_sc) and np.array_equal(ok['end_start'], good_st)
    finite = good_sc > NINF
    same_support = np.array_equal(bad['end_score'] > NINF, finite)
    if not same_support or np.abs(bad['end_score'][finite] - good_sc[finite]).max() > R.kws_bound(len(lp), ok['P']):
        caught.append('bound')
    thr = -1.0 * len(kw)
    if KS.pick_hits_host(bad['end_score'], bad['end_start'], thr, 8) != KS.pick_hits_host(good_sc, good_st, thr, 8):
        caught.append('hit')
    print(defect, caught)
    assert caught, defect
    if defect == 'enter_first':                                          # the scores are the same: only the starts move
        assert caught == ['hit'] and np.array_equal(bad['end_score'], good_sc)
