"""w2l_edit_distance and w2l_nbest_mbr (csrc/edit_distance.hip) against the integer / float64 references of mbr_refs.py, then
the searches' ``mbr=`` end to end against mbr.mbr_select_host applied to the same search's own n-best list.

Integers -- distances, counts, picks, statuses, the copied rows -- are compared exactly.  The risks are sums of non-negative
terms, so their bound is relative: |got - ref| <= c(k) * u * ref with u = 2^-53 and c(k) = 4 k + 4 (DEVICE_EXP_ULP +
HOST_EXP_ULP), derived from the operation count in mbr_refs.risk_bound_c.  test_cpu_mbr.py shows on the host that no case here,
direct or end to end, has two least risks closer than twice that bound unless they are equal by construction, so no case is
excluded from the exact comparison of the picks."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from asg_replay_worker import build_model, synthetic_batch
from direct_helpers import Buf, guards, last_error, p, ratio, record
from mbr_refs import (E2E_HOTWORDS, E2E_K, E2E_LEXICON, E2E_N, E2E_SEEDS, E2E_T, MAX_TOKENS, SMALL, U, cases, e2e_posteriors,
                      e2e_transitions, edit_ops, nbest_ref, risk_bound_c)
from wav2letter_pytorch_amd import _lib as L
from wav2letter_pytorch_amd import mbr
from wav2letter_pytorch_amd.alignment import ctc_forced_align
from wav2letter_pytorch_amd.asg_beam import ASGBeamSearchDecoder, asg_beam_search_gpu, asg_forced_align
from wav2letter_pytorch_amd.beam_search import GPUPrefixBeamSearchDecoder, prefix_beam_search_gpu, search_out_layout
from wav2letter_pytorch_amd.decoder import Decoder, _edit_distance
from wav2letter_pytorch_amd.lexicon import Lexicon

pytestmark = pytest.mark.gpu

CASES = {c['name']: c for c in cases()}
PAIR_CASES = [n for n, c in CASES.items() if c['kind'] == 'pairs']
NBEST_CASES = [(n, u) for n, c in CASES.items() if c['kind'] == 'nbest' for u in c['units']]


@functools.lru_cache(maxsize=None)
def _pairs_reference(name):
    """(d, sub, del, ins) of every pair of the case, computed once"""
    case = CASES[name]
    memo = {}
    return np.array([memo.setdefault((a, b), edit_ops(case['seqs'][a], case['seqs'][b])) for a, b in case['pairs'].tolist()],
                    dtype=np.int32)


def _run_pairs(seqs, pairs, counts=True, max_len=None):
    """w2l_edit_distance itself, on guarded buffers -> (dist [P], counts [P, 3] or None, status [P])"""
    seqs = [np.asarray(s, dtype=np.int32) for s in seqs]
    pairs = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
    offsets = np.zeros(len(seqs) + 1, dtype=np.int32)
    offsets[1:] = np.cumsum([len(s) for s in seqs])
    total, p_n = int(offsets[-1]), len(pairs)
    longest = max(len(s) for s in seqs) if max_len is None else max_len
    tok = Buf((max(total, 1),), torch.int32, np.concatenate(seqs + [np.zeros(0 if total else 1, dtype=np.int32)]))
    off = Buf((len(seqs) + 1,), torch.int32, offsets)
    pr = Buf((p_n, 2), torch.int32, pairs)
    dist, status = Buf((p_n,), torch.int32), Buf((p_n,), torch.int32)
    cnt = Buf((p_n, 3), torch.int32) if counts else None
    assert L.lib.w2l_edit_distance_workspace_bytes(total, len(seqs), p_n, longest) == 0
    rc = L.lib.w2l_edit_distance(p(L, tok), total, p(L, off), len(seqs), p(L, pr), p_n, longest, None, 0, p(L, dist), p(L, cnt),
                                 p(L, status), L.stream_ptr())
    assert rc == 0, last_error(L)
    torch.cuda.synchronize()
    assert guards(tok, off, pr, dist, status, cnt)
    return dist.np(), cnt.np() if counts else None, status.np()


# ------------------------------------------------------------------------------------------------ direct: w2l_edit_distance
@pytest.mark.parametrize('name', PAIR_CASES)
def test_edit_distance_direct(name):
    case = CASES[name]
    ref = _pairs_reference(name)
    dist, cnt, status = _run_pairs(case['seqs'], case['pairs'])
    assert not status.any()
    assert (dist == ref[:, 0]).all(), np.nonzero(dist != ref[:, 0])[0][:8]
    assert (cnt == ref[:, 1:]).all(), np.nonzero((cnt != ref[:, 1:]).any(axis=1))[0][:8]
    if name == 'disjoint':
        lens = np.array([[len(case['seqs'][a]), len(case['seqs'][b])] for a, b in case['pairs']])
        assert (dist == lens.max(axis=1)).all()
    if name == 'identical':
        assert not dist.any() and not cnt.any()
    if name == 'one-pair':                                # without the counts: the same distance, nothing else written
        again, none, _ = _run_pairs(case['seqs'], case['pairs'], counts=False)
        assert none is None and (again == dist).all()


def test_edit_distance_at_the_maximum_length():
    rng = np.random.RandomState(5)
    a, b = rng.randint(0, 4, size=MAX_TOKENS), rng.randint(0, 4, size=MAX_TOKENS)
    big = rng.randint(0, 1000, size=MAX_TOKENS)
    cut = np.concatenate([big[:1000], big[1500:]])        # a block removed: d = na - nb, so 0 substitutions, all deletions
    dist, cnt, status = _run_pairs([a, b, big, cut], [(0, 1), (2, 3), (3, 2)])
    assert not status.any()
    assert dist[0] == _edit_distance(a, b)
    d, s, dl, n = cnt[0].sum(), *cnt[0]
    assert d == dist[0] and MAX_TOKENS - dl + n == MAX_TOKENS
    assert dist[1] == 500 and cnt[1].tolist() == [0, 500, 0]
    assert dist[2] == 500 and cnt[2].tolist() == [0, 0, 500]


def test_edit_distance_refuses_what_is_out_of_range():
    """a sequence longer than max_len, offsets out of order, an index outside the sequences: a status and -1, the other pairs
    of the launch are unharmed; beyond the limit nothing is launched"""
    seqs = [[1, 2, 3], [1, 3], list(range(70))]
    dist, cnt, status = _run_pairs(seqs, [(0, 1), (0, 2), (2, 1), (0, 3), (-1, 0), (1, 0)], max_len=64)
    assert status.tolist() == [0, 1, 1, 2, 2, 0] and dist.tolist() == [1, -1, -1, -1, -1, 1]
    assert cnt[0].tolist() == [0, 1, 0] and cnt[5].tolist() == [0, 0, 1] and (cnt[1:5] == -1).all()
    d = Buf((1,), torch.int32)
    assert L.lib.w2l_edit_distance(p(L, d), 1, p(L, d), 1, p(L, d), 1, MAX_TOKENS + 1, None, 0, p(L, d), None, p(L, d),
                                   L.stream_ptr()) != 0
    assert 'out of range' in last_error(L)


def test_edit_distance_gpu_strings_and_counts():
    dec = Decoder(SMALL)
    refs = ['THE CAT SAT', 'A  B', '', 'ONE TWO THREE', 'SAME']
    hyps = ['THE CAT', 'A B C', 'X', 'ONE THREE TWO', 'SAME']
    for unit, measure in (('word', dec.wer), ('char', dec.cer)):
        dist, counts = mbr.edit_distance_gpu(refs, hyps, unit=unit, counts=True)
        assert dist.tolist() == [measure(r, h) for r, h in zip(refs, hyps)]
        assert (counts.sum(axis=1) == dist).all()
        assert (mbr.edit_distance_gpu(refs, hyps, unit=unit) == dist).all()
    assert mbr.edit_distance_gpu([[1, 2, 3], []], [[1, 3], [4, 4]]).tolist() == [1, 2]


# ---------------------------------------------------------------------------------------------------- direct: w2l_nbest_mbr
def _run_nbest(case, unit):
    """w2l_nbest_mbr itself on the case's hand-built out buffer -> mbr.MbrResult (host arrays)"""
    n, k, t = case['n'], case['k'], case['t']
    lay = search_out_layout(n, k, t, False)
    head = np.concatenate([case['score'].reshape(-1).view(np.uint8), case['len'].reshape(-1).view(np.uint8),
                           np.zeros(4 * n, dtype=np.uint8), case['rows'].reshape(-1).view(np.uint8)])
    assert head.size == lay.beam_bytes
    at = mbr.mbr_offset(lay.beam_bytes)
    sec = mbr.mbr_sections(n, k, t)
    out = Buf((at + sec.total,), torch.uint8)
    out.t[:lay.beam_bytes].copy_(torch.from_numpy(head))
    ws_bytes = L.lib.w2l_nbest_mbr_workspace_bytes(n, k, t)
    ws = Buf((ws_bytes,), torch.uint8)
    cls = mbr.label_classes(case['labels'])
    rc = L.lib.w2l_nbest_mbr(p(L, out), n, k, t, cls.ctypes.data_as(C.c_void_p), len(cls), mbr.UNITS.index(unit), case['repeat'],
                             float(case['scale']), p(L, ws), ws_bytes, C.c_void_p(out.t.data_ptr() + at), L.stream_ptr())
    assert rc == 0, last_error(L)
    torch.cuda.synchronize()
    assert guards(out, ws)
    host = out.np()
    assert (host[:lay.beam_bytes] == head).all()          # the search's results are read, never written
    return mbr.split_mbr(host[at:], n, k, t)


@pytest.mark.parametrize('name,unit', NBEST_CASES)
def test_nbest_mbr_direct(name, unit):
    case = CASES[name]
    ref = nbest_ref(case, unit)
    got = _run_nbest(case, unit)
    for key in ('status', 'dist', 'pick', 'pick_len', 'pick_labels'):
        assert (getattr(got, key) == ref[key]).all(), (key, getattr(got, key), ref[key])
    assert (np.isnan(got.risk) == np.isnan(ref['risk'])).all()
    here = ~np.isnan(ref['risk'])
    c = risk_bound_c(case['k'])
    if here.any():                                        # (no present row anywhere: all NaN, compared above)
        r = record('nbest_mbr.risk', '%s/%s' % (name, unit),
                   ratio(got.risk[here], ref['risk'][here], c * U * ref['risk'][here]))
        assert r <= 1.0, (r, c)
    assert (got.dist == got.dist.transpose(0, 2, 1)).all()


def test_nbest_mbr_refuses_bad_arguments():
    out = Buf((4096,), torch.uint8)
    cls = mbr.label_classes(SMALL)

    def call(n=1, k=2, t=8, a=6, unit=0, repeat=-1, scale=1.0, off=512):
        return L.lib.w2l_nbest_mbr(p(L, out), n, k, t, cls.ctypes.data_as(C.c_void_p), a, unit, repeat, scale, p(L, out), 4096,
                                   C.c_void_p(out.t.data_ptr() + off), L.stream_ptr())

    for kw in (dict(k=65), dict(k=0), dict(unit=2), dict(repeat=6), dict(scale=-1.0), dict(scale=float('nan')), dict(a=0),
               dict(off=516), dict(t=4000)):
        assert call(**kw) != 0, kw
    torch.cuda.synchronize()
    assert guards(out)


# -------------------------------------------------------------------------------------------------------------- end to end
def _variants():
    return (('plain', {}), ('lexicon', dict(lexicon=Lexicon(E2E_LEXICON))),
            ('hotwords', dict(hotwords=E2E_HOTWORDS, hotword_weight=1.0)))


def _check_against_host(search, unit, scale=1.0):
    """``search(**kw)``: the device search on one batch.  Its ``mbr=unit`` results against mbr_select_host on its own n-best"""
    lists = search(nbest=E2E_K, return_weights=True)
    picked = search(mbr=unit, mbr_scale=scale, return_weights=True, return_risks=True)
    ranked = search(mbr=unit, mbr_scale=scale, nbest=E2E_K, return_risks=True)
    moved = 0
    for u, rows in enumerate(lists):
        pick, risks, _ = mbr.mbr_select_host(rows, unit, scale)
        text, weight, risk = picked[u]
        assert (text, weight) == rows[pick], (u, picked[u], rows[pick])
        assert abs(risk - risks[pick]) <= risk_bound_c(E2E_K) * U * risks[pick]
        order = sorted(range(len(rows)), key=lambda i: (ranked_risk(ranked[u], rows, i), i))
        assert [r[:2] for r in ranked[u]] == [rows[i] for i in order]
        got = [r[2] for r in ranked[u]]
        assert got == sorted(got) and got[0] == risk                                          # ascending risk
        for i, g in zip(order, got):
            assert abs(g - risks[i]) <= risk_bound_c(E2E_K) * U * risks[i]
        moved += pick != 0
    assert search(mbr=unit, mbr_scale=scale) == [row[0] for row in picked]
    return moved


def ranked_risk(ranked_rows, rows, i):
    """the device's risk of n-best row i (texts are unique in a beam)"""
    return next(r[2] for r in ranked_rows if r[:2] == rows[i])


@pytest.mark.parametrize('unit', ['word', 'char'])
@pytest.mark.parametrize('seed', E2E_SEEDS)
def test_ctc_search_with_mbr(seed, unit):
    x = torch.from_numpy(e2e_posteriors(seed)).cuda()
    moved = {}
    for name, kw in _variants():
        moved[name] = _check_against_host(functools.partial(prefix_beam_search_gpu, x, SMALL, k=E2E_K, **kw), unit)
        assert prefix_beam_search_gpu(x, SMALL, k=E2E_K, mbr=None, nbest=E2E_K, return_weights=True, **kw) == \
            prefix_beam_search_gpu(x, SMALL, k=E2E_K, nbest=E2E_K, return_weights=True, **kw)
    assert moved['plain'] > 0                             # (shown on the host in test_cpu_mbr.py: a pick that is not rank 0)
    _check_against_host(functools.partial(prefix_beam_search_gpu, x, SMALL, k=E2E_K), unit, scale=0.5)
    one = prefix_beam_search_gpu(x[1], SMALL, k=E2E_K, mbr=unit)
    assert one == prefix_beam_search_gpu(x, SMALL, k=E2E_K, mbr=unit)[1]


@pytest.mark.parametrize('unit', ['word', 'char'])
@pytest.mark.parametrize('seed', E2E_SEEDS)
def test_asg_search_with_mbr(seed, unit):
    x, g = e2e_posteriors(seed, asg=True), e2e_transitions(seed)
    search = functools.partial(asg_beam_search_gpu, x, g, SMALL, k=E2E_K)
    _check_against_host(search, unit)
    assert search(mbr=None, nbest=E2E_K, return_weights=True) == search(nbest=E2E_K, return_weights=True)
    enc = search(mbr=unit, return_encoded=True, return_risks=True)
    plain = search(nbest=E2E_K, return_encoded=True)
    for u in range(E2E_N):
        assert enc[u][:3] in plain[u] and len(enc[u]) == 4
    dec = ASGBeamSearchDecoder(SMALL, transitions=g, k=E2E_K, mbr=unit)
    assert dec.decode(x) == search(mbr=unit)


@pytest.mark.parametrize('seed', E2E_SEEDS)
def test_offsets_are_the_picked_strings(seed):
    p_host = e2e_posteriors(seed)
    x = torch.from_numpy(p_host).cuda()
    sizes = [E2E_T, E2E_T - 7, E2E_T - 3]
    texts, offs = prefix_beam_search_gpu(x, SMALL, k=E2E_K, mbr='word', return_offsets=True, sizes=sizes)
    assert texts == prefix_beam_search_gpu(x, SMALL, k=E2E_K, mbr='word', sizes=sizes)
    ref = ctc_forced_align(x, texts, input_lengths=sizes, log_probs=False, labels=SMALL)
    assert all(texts)
    for u, text in enumerate(texts):
        assert ref.feasible[u] and offs[u].tolist() == ref.starts[u, :len(text)].tolist()
    dec = GPUPrefixBeamSearchDecoder(None, SMALL, k=E2E_K, mbr='word')
    strings, nested = dec.decode(x, torch.tensor(sizes), return_offsets=True)
    assert strings == texts and [o[0].tolist() for o in nested] == [o.tolist() for o in offs]
    # ASG: the pick's encoded row is aligned where w2l_nbest_mbr copied it
    xs, g = e2e_posteriors(seed, asg=True), e2e_transitions(seed)
    texts, offs = asg_beam_search_gpu(xs, g, SMALL, k=E2E_K, mbr='char', return_offsets=True)
    rows = asg_beam_search_gpu(xs, g, SMALL, k=E2E_K, mbr='char', return_encoded=True)
    for u, (text, _, enc) in enumerate(rows):
        assert text == texts[u]
        ref = asg_forced_align(xs[u], g, [list(enc)], repeat_index=0, encoded=True)
        lead = 1 if enc and enc[0] == 0 else 0
        assert offs[u].tolist() == ref.starts[0, lead:len(enc)].tolist() and len(offs[u]) == len(text)


def test_evaluate_error_counts():
    from wav2letter_pytorch_amd.evaluate import evaluate
    model = build_model(criterion='ctc').cuda().eval()
    batch = synthetic_batch(model.labels)
    dec = GPUPrefixBeamSearchDecoder(None, model.labels, k=4, mbr='word',
                                     log_probs=bool(getattr(model, 'infer_log_probs', True)))
    plain_metrics, plain_records = evaluate(model, [batch], decoder=dec)
    metrics, records = evaluate(model, [batch], decoder=dec, error_counts=True)
    assert len(records) == 4 and 'word_sub' not in plain_records[0] and 'test_word_sub' not in plain_metrics
    new = {'%s_%s' % (unit, kind) for unit in ('word', 'char') for kind in ('sub', 'del', 'ins')}
    assert set(metrics) == set(plain_metrics) | {'test_' + key for key in new}              # today's keys, and the six
    host = Decoder(model.labels)
    for unit, measure in (('word', host.wer), ('char', host.cer)):
        total = 0
        for r, q in zip(records, plain_records):
            assert set(r) == set(q) | new
            errors = r[unit + '_sub'] + r[unit + '_del'] + r[unit + '_ins']
            assert errors == r[unit + '_errors'] == measure(r['text'], r['hypothesis'])
            total += errors
        ref_len = sum(r[unit + '_ref'] for r in records)
        assert ref_len > 0
        parts = sum(metrics['test_%s_%s' % (unit, kind)] for kind in ('sub', 'del', 'ins'))
        assert abs(parts - total / ref_len) < 1e-12
        assert abs(parts - metrics['test_wer' if unit == 'word' else 'test_cer']) < 1e-12
