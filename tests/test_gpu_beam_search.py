"""The device prefix beam search (w2l_ctc_beam_search) against the host recursion it restates.

The oracle is beam_search.prefix_beam_search on float64 input: every posterior below is generated in float32 and widened
exactly, so both sides read the same numbers."""
import numpy as np
import pytest
import torch

from wav2letter_pytorch_amd.beam_search import GPUPrefixBeamSearchDecoder, prefix_beam_search, prefix_beam_search_gpu
from wav2letter_pytorch_amd.beam_search import _beam_search_device
from wav2letter_pytorch_amd.data.label_sets import english_labels

pytestmark = pytest.mark.gpu


def _peaky(seed, n, t, a, blank=0, boost=(5.0, 11.0), p_blank=0.6, max_burst=3):
    """blank-dominant synthetic posteriors with bursts of one character, float32 [n, t, a]; each blank frame or burst
    lifts its label's logit by a boost drawn from the range ``boost``"""
    rng = np.random.default_rng(seed)
    logits = rng.standard_normal((n, t, a))
    for u in range(n):
        f = 0
        while f < t:
            if rng.random() < p_blank:
                logits[u, f, blank] += rng.uniform(*boost)
                f += 1
                continue
            c = int(rng.integers(0, a - 1))
            c += c >= blank
            burst = int(rng.integers(1, max_burst + 1))
            logits[u, f:f + burst, c] += rng.uniform(*boost)
            f += burst
    e = np.exp(logits - logits.max(-1, keepdims=True))
    return (e / e.sum(-1, keepdims=True)).astype(np.float32)


def _host(p32, labels, **kw):
    return prefix_beam_search(p32.astype(np.float64), labels, return_weights=True, **kw)


def _check_close(logw, w_host):
    assert w_host > 0
    ref = np.log(w_host)
    assert abs(logw - ref) <= 1e-9 * max(1.0, abs(ref)), (logw, ref)


# ---------------------------------------------------------------------------------------------------------- known answers
def _asr_sample():
    s = np.zeros((10, len(english_labels)))
    s[0, 2] = 0.5
    s[1, 20] = 0.5
    s[2, 19] = 0.5
    s[3:, 0] = 0.5
    return s


def test_sanity():
    assert prefix_beam_search_gpu(_asr_sample(), english_labels) == 'ASR'


def test_inconsistent_sizes():
    with pytest.raises(ValueError):
        prefix_beam_search_gpu(np.zeros((10, len(english_labels) - 1)), english_labels)


def test_beam_is_not_greedy():
    labels = ['_', 'A', 'B', ' ']
    samples = np.array([[0.8, 0.2, 0, 0], [0.6, 0.4, 0, 0]])
    best, logw = prefix_beam_search_gpu(samples, labels, blank_index=0, return_weights=True)
    assert best == 'A'
    assert np.exp(logw) == pytest.approx(0.52)          # (the device reads fp32 posteriors)


def test_class_wrapper():
    assert GPUPrefixBeamSearchDecoder('', english_labels).decode(_asr_sample()) == 'ASR'


def test_pbs_batch_dimensions():
    sample = torch.from_numpy(_asr_sample()).unsqueeze(0)
    assert GPUPrefixBeamSearchDecoder('', english_labels).decode(sample) == ['ASR']
    assert GPUPrefixBeamSearchDecoder('', english_labels).decode(sample.repeat(3, 1, 1).cuda()) == ['ASR'] * 3


def test_negative_input_raises():
    s = _asr_sample()
    s[4, 3] = -0.1
    with pytest.raises(ValueError):
        prefix_beam_search_gpu(s, english_labels)


# ---------------------------------------------------------------------------------------------------------- seeded corpus
CORPUS = [  # (T, k, beta, prune)
    (50, 1, 0, 1e-3), (50, 5, 5, 0.0), (50, 16, 5, 1e-3), (50, 16, 0, 0.0),
    (200, 1, 5, 0.0), (200, 5, 0, 1e-3), (200, 5, 5, 0.0), (200, 16, 5, 1e-3),
    (500, 1, 5, 1e-3), (500, 5, 5, 1e-3), (500, 5, 0, 1e-3), (500, 16, 0, 1e-3),
]


@pytest.mark.parametrize('t,k,beta,prune', CORPUS)
def test_seeded_corpus(t, k, beta, prune):
    labels = english_labels
    p = _peaky(1000 + t + k, 16, t, len(labels))
    res = prefix_beam_search_gpu(torch.from_numpy(p).cuda(), labels, k=k, beta=beta, prune=prune, return_weights=True)
    for u in range(p.shape[0]):
        best, w = _host(p[u], labels, k=k, beta=beta, prune=prune)
        assert w > 1e-250
        assert res[u][0] == best, (u, res[u][0], best)
        _check_close(res[u][1], w)


def test_special_labels_close_and_count_words():
    labels = ['_', 'a', 'b', 'c', ' ', '|', '>']
    closed = words = 0
    for seed in range(4):
        p = _peaky(seed, 8, 120, len(labels), boost=(3.0, 7.0), p_blank=0.5)
        for beta in (2, 5):
            res = prefix_beam_search_gpu(p, labels, k=8, beta=beta, return_weights=True)
            for u in range(p.shape[0]):
                best, w = _host(p[u], labels, k=8, beta=beta)
                assert res[u][0] == best, (seed, beta, u, res[u][0], best)
                _check_close(res[u][1], w)
                closed += best.endswith('>')
                words += '|' in best
    assert closed > 0 and words > 0


def test_duplicate_labels():
    labels = ['_', 'A', 'B', 'A', ' ']
    p = _peaky(7, 8, 80, len(labels), boost=(2.0, 5.0))
    res = prefix_beam_search_gpu(p, labels, k=6, beta=1, return_weights=True)
    for u in range(p.shape[0]):
        best, w = _host(p[u], labels, k=6, beta=1)
        assert res[u][0] == best
        _check_close(res[u][1], w)


def test_frame_without_labels_empties_the_beam():
    p = _peaky(3, 2, 30, len(english_labels))
    p[:, 12] = 0.0
    assert _host(p[0], english_labels)[0] == ''
    assert prefix_beam_search_gpu(p, english_labels) == ['', '']


def test_t2_and_k1():
    labels = ['_', 'A', 'B', ' ']
    p = np.array([[[0.5, 0.3, 0.2, 0.0], [0.1, 0.2, 0.6, 0.1]]], dtype=np.float32)
    for k in (1, 2, 5):
        best, w = _host(p[0], labels, k=k)
        got, logw = prefix_beam_search_gpu(p, labels, k=k, return_weights=True)[0]
        assert got == best
        _check_close(logw, w)


def test_sizes():
    labels = english_labels
    p = _peaky(11, 6, 90, len(labels))
    sizes = [90, 2, 17, 64, 45, 89]
    got = GPUPrefixBeamSearchDecoder('', labels).decode(torch.from_numpy(p), sizes=torch.tensor(sizes))
    assert got == [prefix_beam_search(p[n, :sizes[n]].astype(np.float64), labels) for n in range(6)]
    full = GPUPrefixBeamSearchDecoder('', labels).decode(torch.from_numpy(p))
    assert full == [prefix_beam_search(p[n].astype(np.float64), labels) for n in range(6)]


def test_log_prob_input():
    labels = english_labels
    p = torch.from_numpy(_peaky(5, 16, 200, len(labels))).cuda()
    a = prefix_beam_search_gpu(p, labels, k=5)
    b = prefix_beam_search_gpu(torch.log(p), labels, k=5, log_probs=True)
    assert a == b
    assert GPUPrefixBeamSearchDecoder('', labels, log_probs=True).decode(torch.log(p)) == a


def test_long_utterances_do_not_underflow():
    labels = english_labels
    p = _peaky(9, 4, 2000, len(labels), boost=(9.0, 9.0), p_blank=0.7)
    assert np.median(p.max(-1)) > 0.98
    got = prefix_beam_search_gpu(torch.from_numpy(p).cuda(), labels, k=5, return_weights=True)
    for u in range(p.shape[0]):
        best, w = _host(p[u], labels, k=5)
        assert best != '' and got[u][0] == best
        _check_close(got[u][1], w)


def test_nbest():
    labels = english_labels
    p = _peaky(13, 4, 150, len(labels))
    best = prefix_beam_search_gpu(p, labels, k=8)
    lists = prefix_beam_search_gpu(p, labels, k=8, nbest=8)
    for b, lst in zip(best, lists):
        assert lst[0][0] == b
        scores = [s for _, s in lst]
        assert all(x >= y for x, y in zip(scores, scores[1:]))
        assert len({s for s, _ in lst}) == len(lst) > 1


def test_deterministic():
    labels = english_labels
    p = torch.from_numpy(_peaky(17, 32, 300, len(labels))).cuda()
    a = _beam_search_device(p, labels, 0, 16, 5, 1e-3, '>', None, False)
    b = _beam_search_device(p, labels, 0, 16, 5, 1e-3, '>', None, False)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()


def test_limits_are_errors():
    with pytest.raises(Exception, match='beam width'):
        prefix_beam_search_gpu(_asr_sample(), english_labels, k=65)
    labels = [chr(0x100 + i) for i in range(129)]
    with pytest.raises(Exception, match='labels'):
        prefix_beam_search_gpu(np.full((4, 129), 1 / 129, dtype=np.float32), labels)
