"""The host model of CTC forced alignment (alignment.viterbi_align_host) against brute force, the pinned tie rules, the
reference-generated greedy fixture, and what of ctc_forced_align / get_time_per_word needs no device."""
import itertools
import os

import numpy as np
import pytest
import torch

from wav2letter_pytorch_amd.alignment import ctc_forced_align, viterbi_align_host
from wav2letter_pytorch_amd.beam_search import get_time_per_word

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def _collapse(path, blank=0):
    out, prev = [], None
    for c in path:
        if c != prev and c != blank:
            out.append(c)
        prev = c
    return tuple(out)


# ------------------------------------------------------------------------------------------------------------- brute force
def test_host_model_against_every_path():
    """A = 3, every T in 2..6: all A**T paths grouped by collapsed string; for every string the host score is the best
    enumerated score (1e-12) and the path is that path.  Continuous Dirichlet draws: ties are a null event."""
    rng = np.random.default_rng(0)
    pairs = 0
    for t_n in range(2, 7):
        paths = np.array(list(itertools.product(range(3), repeat=t_n)))
        keys = [_collapse(p) for p in paths]
        for _ in range(40):
            lp = np.log(rng.dirichlet(np.ones(3), size=t_n))
            scores = lp[np.arange(t_n), paths].sum(1)
            best = {}
            for i, key in enumerate(keys):
                if key not in best or scores[i] > scores[best[key]]:
                    best[key] = i
            for key, i in best.items():
                got = viterbi_align_host(lp, list(key))
                assert got.feasible
                assert abs(got.score - scores[i]) <= 1e-12, (t_n, key)
                assert got.path.tolist() == paths[i].tolist(), (t_n, key)
                # starts / ends restate the path: first and last frame of each token's run
                pos = [f for f in range(t_n) if paths[i][f] != 0 and (f == 0 or paths[i][f - 1] != paths[i][f])]
                assert got.starts.tolist() == pos
                last = [f for f in range(t_n) if paths[i][f] != 0 and (f == t_n - 1 or paths[i][f + 1] != paths[i][f])]
                assert got.ends.tolist() == last
                pairs += 1
    assert pairs > 3000


# --------------------------------------------------------------------------------------------------------------- tie rules
def _lp(rows):
    return np.log(np.array(rows, dtype=np.float64))


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_tie_stay_before_advance(dtype):
    # target 'a' on uniform frames: every path that spells 'a' scores the same.  Stay wins every tie, the last label wins
    # the end: the walk ends in a's state and stays there back to frame 1; at frame 0 states 0 and 1 ... a's state at
    # frame 1 has predecessors a (stay) and blank (s-1) equal -> stay.
    lp = _lp([[0.5, 0.5]] * 4)
    got = viterbi_align_host(lp, [1], dtype=dtype)
    assert got.path.tolist() == [1, 1, 1, 1]
    assert got.starts.tolist() == [0] and got.ends.tolist() == [3]


def test_tie_s_minus_1_before_s_minus_2():
    # target 'ab', 3 frames, b all but impossible at frame 0, frames 1 and 2 uniform: a three-way tie at frame 2
    lp = _lp([[0.5, 0.5, 1e-300], [1 / 3, 1 / 3, 1 / 3], [1 / 3, 1 / 3, 1 / 3]])
    got = viterbi_align_host(lp, [1, 2])
    # end: state 3 (b) vs state 4 (blank) tie -> b.  b's state at frame 2: stay = lp0(a) + lp1(b) equals s-1 (a, blank) and
    # s-2 (a, a): stay wins -> b at frame 1; there stay = -690 (b at frame 0), s-1 = -inf, s-2 = a at frame 0 wins.
    assert got.path.tolist() == [1, 2, 2]
    # stay is not available (b impossible at frame 1): s-1 (the blank between) must win over s-2 (straight from a)
    lp = _lp([[0.5, 0.5, 1e-300], [0.5, 0.5, 1e-300], [1 / 3, 1 / 3, 1 / 3]])
    lp[1, 2] = -np.inf
    lp[0, 2] = -np.inf
    got = viterbi_align_host(lp, [1, 2])
    # frame 2, state 3: stay = -inf, s-1 = state 2 at frame 1 = lp0(a) + lp1(blank), s-2 = state 1 at frame 1 = lp0(a) + lp1(a)
    # (stay; equal to blank->a), equal -> s-1; state 2 at frame 1: stay -inf, s-1 = state 1 at frame 0 -> a
    assert got.path.tolist() == [1, 0, 2]
    assert got.starts.tolist() == [0, 2] and got.ends.tolist() == [0, 2]


def test_tie_end_prefers_last_label():
    lp = _lp([[0.5, 0.5], [0.5, 0.5]])
    got = viterbi_align_host(lp, [1])
    assert got.path.tolist() == [1, 1]          # (a, blank) scores the same and loses
    # a strictly better trailing blank wins
    lp = _lp([[0.5, 0.5], [0.6, 0.4]])
    assert viterbi_align_host(lp, [1]).path.tolist() == [1, 0]


def test_minus_inf_stays_minus_inf_and_zero_probabilities():
    lp = np.log(np.array([[0.5, 0.5, 0.0], [0.5, 0.0, 0.5], [1.0, 0.0, 0.0]]))
    got = viterbi_align_host(lp, [1, 2])
    assert got.feasible and got.path.tolist() == [1, 2, 0]
    assert got.score == pytest.approx(np.log(0.25))
    # every path through a zero: infeasible
    got = viterbi_align_host(lp, [2, 1])
    assert not got.feasible and got.score == -np.inf
    assert got.path.tolist() == [-1, -1, -1] and got.starts.tolist() == [-1, -1] and got.ends.tolist() == [-1, -1]


def test_empty_target_one_frame_and_infeasible():
    rng = np.random.default_rng(1)
    lp = np.log(rng.dirichlet(np.ones(4), size=5))
    got = viterbi_align_host(lp, [])
    assert got.feasible and got.path.tolist() == [0] * 5 and got.starts.size == 0 and got.ends.size == 0
    assert got.score == pytest.approx(lp[:, 0].sum())
    got = viterbi_align_host(lp, [], blank=2)
    assert got.path.tolist() == [2] * 5
    one = viterbi_align_host(lp[:1], [3])
    assert one.feasible and one.path.tolist() == [3] and one.starts.tolist() == [0] and one.ends.tolist() == [0]
    assert one.score == lp[0, 3]
    assert viterbi_align_host(lp[:1], []).path.tolist() == [0]
    # 'aa' needs a blank between: three frames at least
    assert not viterbi_align_host(lp[:2], [1, 1]).feasible
    got = viterbi_align_host(lp[:3], [1, 1])
    assert got.feasible and got.path.tolist() == [1, 0, 1]
    assert not viterbi_align_host(lp[:1], [1, 2]).feasible
    with pytest.raises(ValueError):
        viterbi_align_host(lp, [0])
    with pytest.raises(ValueError):
        viterbi_align_host(lp, [4])


# ------------------------------------------------------------------------------------------------- the reference's fixture
@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_greedy_fixture_offsets(dtype):
    """tests/golden/greedy_cases.npz (written by the reference's GreedyDecoder): aligning each utterance's collapsed argmax
    string over its sizes[n] frames gives starts == offsets where the frame maxima are unique (utterances 0, 1, 3).
    Utterance 2 holds an exactly uniform frame (frame 5): argmax takes the lowest index there, Viterbi need not, so for it
    the score must equal the argmax path's score and the path must collapse to the string."""
    z = np.load(os.path.join(GOLD, 'greedy_cases.npz'), allow_pickle=True)
    labels = list(z['labels'])
    first = {}
    for i, ch in enumerate(labels):
        first.setdefault(ch, i)
    for n in range(4):
        size = int(z['sizes'][n])
        p = z['probs'][n, :size].astype(dtype)
        with np.errstate(divide='ignore'):
            lp = np.log(p)
        target = [first[ch] for ch in str(z['strings'][n])]
        got = viterbi_align_host(lp, target, dtype=dtype)
        assert got.feasible
        assert _collapse(got.path.tolist()) == tuple(target)
        if n == 2:
            am = z['argmax'][n, :size]
            ref = lp[np.arange(size), am].astype(np.float64).sum()
            assert abs(float(got.score) - ref) <= (1e-9 if dtype is np.float64 else 2 * size * 2.0 ** -24 * abs(ref))
        else:
            assert got.starts.tolist() == list(z['offsets'][n]), n


# --------------------------------------------------------------------------------------------------------- word timestamps
def test_get_time_per_word_end_offsets():
    text = 'ab  cd e'
    offsets = [0, 3, 5, 6, 8, 11, 12, 20]
    ends = [2, 4, 5, 7, 10, 11, 19, 22]
    assert get_time_per_word(text, offsets) == [('ab', 0, 3), ('cd', 8, 11), ('e', 20, 20)]
    assert get_time_per_word(text, offsets, 2.0) == [('ab', 0, 6), ('cd', 16, 22), ('e', 40, 40)]
    assert get_time_per_word(text, offsets, end_offsets=ends) == [('ab', 0, 4), ('cd', 8, 11), ('e', 20, 22)]
    assert get_time_per_word(text, offsets, 0.5, end_offsets=ends) == [('ab', 0, 2), ('cd', 4, 5.5), ('e', 10, 11)]
    assert get_time_per_word('', [], end_offsets=[]) == []
    # IntTensors, as the decoders return them
    got = get_time_per_word('a b', torch.IntTensor([1, 2, 4]), 1.0, end_offsets=torch.IntTensor([1, 3, 6]))
    assert [(w, int(s), int(e)) for w, s, e in got] == [('a', 1, 1), ('b', 4, 6)]
    with pytest.raises(AssertionError):
        get_time_per_word('ab', [0, 1], end_offsets=[0])


# ------------------------------------------------------------------------------------------------- validation, no device
def test_forced_align_validation_without_device():
    lp = torch.zeros(2, 5, 4)
    with pytest.raises(ValueError, match='not in the labels'):
        ctc_forced_align(lp, ['ab', 'zz'], labels=['_', 'a', 'b', 'c'])
    with pytest.raises(ValueError, match='need ``labels``'):
        ctc_forced_align(lp, ['ab', 'a'])
    with pytest.raises(ValueError, match='labels: 3'):
        ctc_forced_align(lp, ['ab', 'a'], labels=['_', 'a', 'b'])
    with pytest.raises(ValueError, match='blank'):
        ctc_forced_align(lp, [[1], [2]], blank=4)
    with pytest.raises(ValueError, match='2 utterances'):
        ctc_forced_align(lp, [[1]])
    with pytest.raises(ValueError, match='input_lengths'):
        ctc_forced_align(lp, [[1], [2]], input_lengths=[5, 6])
    with pytest.raises(ValueError, match='input_lengths'):
        ctc_forced_align(lp, [[1], [2]], input_lengths=[0, 5])
    with pytest.raises(ValueError, match='input_lengths holds 1'):
        ctc_forced_align(lp, [[1], [2]], input_lengths=[5])
    with pytest.raises(ValueError, match='target_lengths'):
        ctc_forced_align(lp, torch.ones(2, 3, dtype=torch.int64), target_lengths=[4, 1])
    with pytest.raises(ValueError, match='target_lengths'):
        ctc_forced_align(lp, [[1], [2]], target_lengths=[1, 1])
    with pytest.raises(ValueError, match='integers'):
        ctc_forced_align(lp, np.ones((2, 3), dtype=np.float32))
    with pytest.raises(ValueError, match='shape'):
        ctc_forced_align(torch.zeros(5), [[1]])
    with pytest.raises(ValueError, match='out of range'):
        ctc_forced_align(lp, np.ones((2, 4096), dtype=np.int64))


def test_names_are_reachable():
    import wav2letter_pytorch_amd as pkg
    from wav2letter_pytorch_amd import alignment, decoder
    assert pkg.ctc_forced_align is alignment.ctc_forced_align and pkg.viterbi_align_host is alignment.viterbi_align_host
    assert decoder.ctc_forced_align is alignment.ctc_forced_align
    assert callable(decoder.Decoder.align)
