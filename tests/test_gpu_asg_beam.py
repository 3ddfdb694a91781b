"""w2l_asg_beam_search, without and with lm, against the host restatement (asg_beam.asg_prefix_beam_search): strings and
n-best order identical, scores within 1e-9 * max(1, |ref|) -- the margin the CTC beam tests use for the same fp64 log
arithmetic.  Inputs are generated in float32 and widened exactly for the host."""
import functools

import numpy as np
import pytest
import torch

from asg_beam_refs import SMALL_LABELS, brute_masses, gen_arpa, log_softmax_scores, small_case, transitions, word_scores
from wav2letter_pytorch_amd.asg_beam import (ASGBeamSearchDecoder, ASGBeamSearchLMDecoder, _search_device, _transitions_on,
                                             asg_beam_search_gpu, asg_prefix_beam_search)
from wav2letter_pytorch_amd.data.label_sets import english_labels

pytestmark = pytest.mark.gpu


def _close(got, ref):
    return abs(got - ref) <= 1e-9 * max(1.0, abs(ref))


def _weigh(lm):
    return functools.lru_cache(maxsize=None)(lambda s: 10 ** lm.score(s))


def _compare(x, g, labels, k, beta, prune=1e-3, sizes=None, lm=None, alpha=0.3, nbest=None):
    """device n-best lists of a batch (or of one utterance) against the host's, utterance by utterance -> the device lists"""
    nbest = nbest or k
    single = x.ndim == 2
    got = asg_beam_search_gpu(x, g, labels, k=k, beta=beta, prune=prune, sizes=sizes, nbest=nbest, lm=lm, alpha=alpha,
                              return_encoded=True, return_weights=True)
    rows = [got] if single else got
    rows = [row if nbest > 1 else [row] for row in rows]
    for u, row in enumerate(rows):
        xu = x if single else x[u]
        tn = xu.shape[0] if sizes is None else int(sizes[u])
        ref = asg_prefix_beam_search(xu[:tn], g, labels, k=k, beta=beta, prune=prune, nbest=nbest, alpha=alpha,
                                     lm=None if lm is None else _weigh(lm), return_encoded=True, return_weights=True)
        ref = ref if nbest > 1 else [ref]
        assert [(t, e) for t, _, e in row] == [(t, e) for t, _, e in ref], (u, row[:3], ref[:3])
        for (_, w, e), (_, wr, _) in zip(row, ref):
            assert _close(w, wr), (u, e, w, wr)
    return rows


@pytest.mark.parametrize('seed', range(3))
def test_exhaustive_case(seed):
    x, g = small_case(seed)
    x, g = x.astype(np.float32), g.astype(np.float32)
    rows = _compare(x, g, SMALL_LABELS, 64, 0, prune=0)
    masses, _, _ = brute_masses(x.astype(np.float64), g.astype(np.float64))
    assert len(rows[0]) == 45
    for _, w, e in rows[0]:
        assert _close(w, masses[e]), (e, w, masses[e])


@pytest.mark.parametrize('beta', [0, 5])
@pytest.mark.parametrize('t,k', [(2, 1), (37, 5), (150, 32)])
def test_english_labels(t, k, beta):
    x = log_softmax_scores(100 + t, (t, 29))
    g = transitions(7, 29)
    rows = _compare(x, g, english_labels, k, beta)
    assert len(rows[0]) == k


def test_batch_with_sizes_equals_single_utterances():
    x = log_softmax_scores(3, (3, 40, 29))
    g = transitions(8, 29)
    sizes = [40, 23, 1]
    rows = _compare(x, g, english_labels, 8, 5, sizes=sizes)
    for u in range(3):
        alone = asg_beam_search_gpu(x[u, :sizes[u]], g, english_labels, k=8, beta=5, nbest=8, return_encoded=True)
        assert alone == rows[u]
    assert len(rows[2]) == 8 and all(len(e) == 1 for _, _, e in rows[2])


def test_lds_limit_64_labels_64_slots():
    labels = ['_'] + [chr(0x100 + i) for i in range(62)] + [' ']
    assert len(set(labels)) == 64
    x = log_softmax_scores(4, (8, 64), scale=2.0)
    g = transitions(9, 64)
    rows = _compare(x, g, labels, 64, 5, prune=1e-4)
    assert len(rows[0]) == 64
    with pytest.raises(ValueError, match='out of range'):
        asg_beam_search_gpu(x, g, labels, k=65, nbest=1)
    with pytest.raises(ValueError):
        asg_beam_search_gpu(np.zeros((4, 65), dtype=np.float32), None, [str(i) for i in range(65)])


@pytest.mark.parametrize('with_lm', [False, True])
def test_english_labels_64_slots(tmp_path, with_lm):
    """k = 64 with 29 labels: 60,836 B of dynamic LDS, under 64 KiB on its own and over it with the kernel's static state"""
    x = word_scores(51, 1, 24, english_labels)[0]
    g = transitions(17, 29, scale=0.3)
    lm = gen_arpa(tmp_path / 'm.arpa', 6, 2) if with_lm else None
    rows = _compare(x, g, english_labels, 64, 5, lm=lm, alpha=1.0)
    assert len(rows[0]) == 64


def test_a_frame_without_a_finite_score_empties_the_beam():
    """as on the host: '' with weight -inf and status 0; with offsets, empty offsets"""
    x = log_softmax_scores(15, (2, 12, 29))
    x[1, 5, :] = -np.inf
    g = transitions(18, 29)
    assert asg_prefix_beam_search(x[1], g, english_labels, k=4, nbest=4, return_weights=True) == [('', -np.inf)]
    got = asg_beam_search_gpu(x, g, english_labels, k=4, nbest=4)
    assert got[1] == [('', -np.inf)] and len(got[0]) == 4 and got[0][0][0]
    texts, offs = asg_beam_search_gpu(x, g, english_labels, k=4, return_offsets=True)
    assert texts == [got[0][0][0], ''] and offs[1].tolist() == [] and len(offs[0]) == len(texts[0])
    dec = ASGBeamSearchDecoder(english_labels, transitions=g, k=4)
    strings, offsets = dec.decode(torch.from_numpy(x).cuda(), return_offsets=True)
    assert strings == texts and offsets[1][0].tolist() == []


def test_long_utterance_scores_are_finite():
    x = log_softmax_scores(5, (1200, 29), scale=2.0)
    got = asg_beam_search_gpu(x, transitions(10, 29), english_labels, k=5, beta=5, nbest=5)
    assert len(got) == 5 and all(np.isfinite(w) and w < -100 for _, w in got)


def test_two_runs_are_byte_equal():
    x = torch.from_numpy(log_softmax_scores(6, (2, 90, 29))).cuda()
    g = _transitions_on(transitions(11, 29), 29, x.device)
    runs = [_search_device(x, g, None, english_labels, 0, 16, 5.0, 1e-3, None, 0.3, False) for _ in range(2)]
    (s0, l0, i0, _, _), (s1, l1, i1, _, _) = runs
    assert s0.tobytes() == s1.tobytes() and l0.tobytes() == l1.tobytes() and (l0 > 0).all()
    for u in range(2):
        for r in range(16):
            assert i0[u, r, :l0[u, r]].tobytes() == i1[u, r, :l1[u, r]].tobytes()


def test_forbidden_transitions_change_the_result():
    x = log_softmax_scores(12, (30, 29))
    g = transitions(13, 29)
    free = _compare(x, g, english_labels, 8, 0)[0]
    gf = g.copy()
    first = free[0][2]
    for u, v in zip(first, first[1:]):
        gf[u, v] = -1e4                                   # forbid every transition the best hypothesis takes
    barred = _compare(x, gf, english_labels, 8, 0)[0]
    assert barred[0][2] != first
    taken = set(zip(first, first[1:]))
    assert not taken & set(zip(barred[0][2], barred[0][2][1:]))


def test_nan_scores_are_reported():
    x = log_softmax_scores(14, (10, 29))
    x[4, 3] = np.nan
    with pytest.raises(ValueError, match='NaN'):
        asg_beam_search_gpu(x, None, english_labels)


# ------------------------------------------------------------------------------------------------------------------- LM
LM_CASES = [(1, 0.3, 5, 5, 50), (2, 1.0, 0, 16, 50), (3, 2.5, 5, 8, 40)]   # (order, alpha, beta, k, T)


@pytest.mark.parametrize('order,alpha,beta,k,t', LM_CASES)
def test_lm_against_host(tmp_path, order, alpha, beta, k, t):
    lm = gen_arpa(tmp_path / 'm.arpa', 20 + order, order)
    x = word_scores(30 + order, 3, t, english_labels)
    g = transitions(14, 29, scale=0.3)
    _compare(x, g, english_labels, k, beta, lm=lm, alpha=alpha)           # (the full k-best list)


def test_lm_alpha_zero_equals_the_lm_free_launch(tmp_path):
    lm = gen_arpa(tmp_path / 'm.arpa', 5, 2)
    x = word_scores(41, 2, 40, english_labels)
    g = transitions(15, 29, scale=0.3)
    kw = dict(k=8, beta=5, nbest=8, return_encoded=True)
    assert asg_beam_search_gpu(x, g, english_labels, lm=lm, alpha=0.0, **kw) == asg_beam_search_gpu(x, g, english_labels, **kw)


def test_lm_changes_the_text_and_spells_doubled_letters(tmp_path):
    lm = gen_arpa(tmp_path / 'm.arpa', 17, 3)
    x = word_scores(33, 12, 45, english_labels)
    g = transitions(16, 29, scale=0.3)
    with_lm = [row[0] for row in _compare(x, g, english_labels, 8, 1, lm=lm, alpha=2.5, nbest=1)]
    without = asg_beam_search_gpu(x, g, english_labels, k=8, beta=1)
    assert sum(a[0] != b for a, b in zip(with_lm, without)) >= 3
    # a repeat label after a letter inside a word: the LM state spelled the letter again (the host scored the decoded text)
    doubled = [e for _, _, e in with_lm if any(v == 0 and i > 0 and e[i - 1] not in (0, 28) for i, v in enumerate(e))]
    assert doubled, [t for t, _, _ in with_lm]
    # lm_log10 of every result is ArpaLM.score of its text, bit for bit
    xs = torch.from_numpy(x).cuda()
    gd = _transitions_on(g, 29, xs.device)
    _, lengths, idx, lm_log10, _ = _search_device(xs, gd, None, english_labels, 0, 8, 1.0, 1e-3, lm, 2.5, False)
    from wav2letter_pytorch_amd.asg_beam import _text
    for u in range(12):
        for r in range(8):
            s = _text(idx[u, r, :lengths[u, r]], english_labels, 0)
            want = np.float32(lm.score(s.strip(' '))) if s.replace(' ', '') else np.float32(0)
            assert lm_log10[u, r].tobytes() == want.tobytes(), (u, r, s)


def test_decoder_classes(tmp_path):
    lm = gen_arpa(tmp_path / 'm.arpa', 17, 2)
    x = torch.from_numpy(word_scores(34, 2, 30, english_labels)).cuda()
    g = torch.from_numpy(transitions(16, 29, scale=0.3))
    dec = ASGBeamSearchDecoder(english_labels, transitions=g, k=6, beta=1)
    want = asg_beam_search_gpu(x, g, english_labels, k=6, beta=1)
    assert dec.decode(x) == want and dec.decode(x[0]) == want[:1]
    assert dec.decode(x, torch.tensor([30, 12])) == asg_beam_search_gpu(x, g, english_labels, k=6, beta=1, sizes=[30, 12])
    dlm = ASGBeamSearchLMDecoder(str(tmp_path / 'm.arpa'), english_labels, transitions=g, k=6, alpha=1.5, beta=1)
    assert dlm.decode(x) == asg_beam_search_gpu(x, g, english_labels, k=6, beta=1, lm=lm, alpha=1.5)
    assert dec.decode(x, transitions=torch.zeros(29, 29)) == asg_beam_search_gpu(x, None, english_labels, k=6, beta=1)


# ----------------------------------------------------------------------------------------------------------- end to end
def test_end_to_end_transcribe_and_evaluate(tmp_path):
    from asg_replay_worker import build_model, synthetic_batch
    from wav2letter_pytorch_amd.asg import ASGDecoder
    from wav2letter_pytorch_amd.evaluate import evaluate
    model = build_model().cuda().eval()
    with torch.no_grad():
        model.criterion.transitions.copy_(torch.from_numpy(transitions(21, 29, scale=0.2)))
    gen_arpa(tmp_path / 'm.arpa', 3, 2, letters=''.join(model.labels[2:7]))
    batch = synthetic_batch(model.labels)
    wave = (0.1 * np.random.default_rng(3).standard_normal(8000)).astype(np.float32)
    for dec in (ASGBeamSearchDecoder(model.labels, transitions=model.criterion, k=4),
                ASGBeamSearchLMDecoder(str(tmp_path / 'm.arpa'), model.labels, transitions=model.criterion, k=4)):
        hyps = model.transcribe([wave, wave[:6000]], decoder=dec)
        assert len(hyps) == 2 and all(isinstance(h, str) for h in hyps)
        metrics, records = evaluate(model, [batch], decoder=dec)
        assert len(records) == 4 and all(np.isfinite(metrics[k]) for k in ('test_loss', 'test_cer', 'test_wer'))
        assert all(isinstance(r['hypothesis'], str) for r in records)
    # k = 1 without pruning and with zero transitions on one-hot-like emissions is the Viterbi decoder
    rng = np.random.default_rng(8)
    path = rng.integers(0, 29, size=(3, 40))
    x = np.full((3, 40, 29), -12.0, dtype=np.float32)
    np.put_along_axis(x, path[..., None], -0.01, axis=-1)
    xs = torch.from_numpy(x).cuda()
    sizes = torch.tensor([40, 31, 17])
    greedy = ASGDecoder(model.labels).decode(xs, sizes, return_offsets=True)
    beam = ASGBeamSearchDecoder(model.labels, k=1, prune=0).decode(xs, sizes, return_offsets=True)
    assert beam[0] == greedy[0]
    for a, b in zip(beam[1], greedy[1]):
        assert a[0].tolist() == b[0].tolist()
