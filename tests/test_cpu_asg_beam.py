"""The host restatements of the ASG prefix beam search and of the ASG forced alignment (asg_beam.asg_prefix_beam_search,
asg_viterbi_align_host) against brute force over every frame path, the test CLI's new decoder values, and the host-side
answers of the new entry points.  No GPU."""
import math

import numpy as np
import pytest

from asg_beam_refs import SMALL_LABELS, brute_align, brute_masses, logsumexp, path_score, small_case, text_of
from wav2letter_pytorch_amd.asg import collapse_frames, encode_repeats
from wav2letter_pytorch_amd.asg_beam import asg_prefix_beam_search, asg_viterbi_align_host


@pytest.mark.parametrize('seed', range(8))
def test_exhaustive_identity(seed):
    """A = 3, T = 4, k = 64, prune = 0, beta = 0: the beam holds all 45 hypotheses, every mass is the brute-force sum over the
    81 frame paths, the best is the brute-force best and the masses add up to Z_full"""
    x, g = small_case(seed)
    masses, z_full, _ = brute_masses(x, g)
    assert len(masses) == 45
    got = asg_prefix_beam_search(x, g, SMALL_LABELS, k=64, prune=0, beta=0, nbest=64, return_encoded=True)
    assert len(got) == 45 and {e for _, _, e in got} == set(masses)
    for text, w, e in got:
        assert text == text_of(e, SMALL_LABELS)
        assert abs(w - masses[e]) <= 1e-12, (e, w, masses[e])
    assert [w for _, w, _ in got] == sorted((w for _, w, _ in got), reverse=True)
    assert got[0][2] == max(masses, key=masses.get)
    assert abs(logsumexp([w for _, w, _ in got]) - z_full) <= 1e-12
    assert asg_prefix_beam_search(x, g, SMALL_LABELS, k=64, prune=0, beta=0) == got[0][0]
    assert asg_prefix_beam_search(x, g, SMALL_LABELS, k=64, prune=0, beta=0, return_weights=True) == got[0][:2]


SEARCH_BEATS_VITERBI_SEEDS = (1, 19, 38)


@pytest.mark.parametrize('seed', SEARCH_BEATS_VITERBI_SEEDS)
def test_search_differs_from_viterbi(seed):
    """fixed draws where the most probable hypothesis is not the one the best single frame path reads"""
    x, g = small_case(seed)
    masses, _, best_path = brute_masses(x, g)
    viterbi_text = text_of(collapse_frames(best_path)[0], SMALL_LABELS)
    text, w, e = asg_prefix_beam_search(x, g, SMALL_LABELS, k=64, prune=0, beta=0, return_encoded=True)
    assert e == max(masses, key=masses.get)
    assert text != viterbi_text, (text, viterbi_text)


def test_leading_repeat_is_dropped_from_the_text_but_kept_as_an_entry():
    x = np.array([[3.0, 1.0, -4.0], [-4.0, 3.0, -4.0]])                   # frame 0 prefers the repeat label, frame 1 'a'
    got = asg_prefix_beam_search(x, np.zeros((3, 3)), SMALL_LABELS, k=16, prune=0, beta=0, nbest=16, return_encoded=True)
    by_e = {e: (text, w) for text, w, e in got}
    assert got[0][2] == (0, 1) and got[0][0] == 'a'
    assert by_e[(1,)][0] == 'a' and by_e[(0,)][0] == ''
    assert abs(by_e[(0, 1)][1] - 6.0) <= 1e-12 and abs(by_e[(1,)][1] - 4.0) <= 1e-12
    assert [text for text, _, _ in got].count('a') >= 2


def test_pruning_keeps_the_argmax():
    """prune = 0.999: no log-probability passes, so every frame extends by its argmax alone and the beam never empties"""
    rng = np.random.default_rng(5)
    z = rng.standard_normal((12, 3))
    x = z - np.log(np.exp(z).sum(-1, keepdims=True))
    assert (x < math.log(0.999)).all()
    g = rng.standard_normal((3, 3))
    got = asg_prefix_beam_search(x, g, SMALL_LABELS, k=5, prune=0.999, beta=0, nbest=5, return_encoded=True)
    path = x.argmax(-1)
    assert len(got) == 1 and got[0][2] == tuple(collapse_frames(path)[0])
    assert abs(got[0][1] - path_score(x, g, path)) <= 1e-12


def test_lm_weight_once_per_closed_word(tmp_path):
    """test_beam_width_changes' bigram: with every hypothesis in the beam, the mass of a hypothesis moves by alpha * ln 10 *
    (the LM score of its text at each word it closes), and of one that closes no word by nothing"""
    from wav2letter_pytorch_amd.ngram_lm import ArpaLM
    (tmp_path / 'a.arpa').write_text('\\data\\\nngram 1=4\nngram 2=2\n\n\\1-grams:\n-1\t<unk>\n-99\t<s>\t0\n0\t</s>\n'
                                     '-1\tA\t0\n\n\\2-grams:\n-0.30103\t<s> A\n0\tA </s>\n\n\\end\\\n')
    arpa = ArpaLM(str(tmp_path / 'a.arpa'))
    labels = ['_', 'A', ' ']
    x, g = small_case(11, 3, 4)
    calls = []

    def lm(s):
        calls.append(s)
        return 10 ** arpa.score(s)

    kw = dict(k=64, prune=0, beta=0, nbest=64, return_encoded=True)
    plain = {e: w for _, w, e in asg_prefix_beam_search(x, g, labels, **kw)}
    alpha = 0.7
    with_lm = {e: w for _, w, e in asg_prefix_beam_search(x, g, labels, lm=lm, alpha=alpha, **kw)}
    assert set(plain) == set(with_lm) and len(plain) == 45
    ln10 = math.log(10)

    def closed_words(e):
        """the LM scores of the texts at which the hypothesis closes a word: a space after a text that does not end in one"""
        total = 0.0
        for j in range(1, len(e)):
            s = text_of(e[:j], labels)
            if e[j] == 2 and s.strip(' ') and s[-1] != ' ':
                total += arpa.score(s.strip(' '))
        return total

    a, aa, unk = arpa.score('A'), arpa.score('A A'), arpa.score('AA')
    assert closed_words((1, 2)) == a and closed_words((1, 2, 1, 2)) == a + aa and closed_words((1, 0, 2)) == unk
    assert closed_words((1, 2, 0, 2)) == a and closed_words((2, 0, 2)) == 0 and closed_words((0, 1, 2, 1)) == a
    for e in plain:
        want = alpha * ln10 * closed_words(e)
        assert abs(with_lm[e] - plain[e] - want) <= 1e-12, (e, with_lm[e] - plain[e], want)
    assert {'A', 'A A', 'AA'} <= set(calls)
    # in the spirit of test_beam_width_changes: the LM's dislike of the lone word 'A' decides a close call
    x2 = np.log(np.array([[0.1, 0.8, 0.1], [0.1, 0.1, 0.8], [0.1, 0.1, 0.8]]))
    assert asg_prefix_beam_search(x2, None, labels, k=8, prune=0, beta=0, alpha=0) == 'A '
    assert asg_prefix_beam_search(x2, None, labels, lm=lambda s: 1e-3 if s == 'A' else 1.0, k=8, prune=0, beta=0,
                                  alpha=1) != 'A '


def test_align_host_against_brute_force():
    rng = np.random.default_rng(2)
    for trial in range(12):
        x, g = 2.0 * rng.standard_normal((5, 3)), rng.standard_normal((3, 3))
        for enc in ([1], [0], [1, 2], [1, 0], [0, 1], [2, 1, 2], [1, 0, 1], [0, 2, 0]):
            res = asg_viterbi_align_host(x, g, enc, encoded=True)
            want = brute_align(x, g, enc)
            assert res.feasible and abs(float(res.score) - want) <= 1e-12
            assert collapse_frames(res.path)[0] == enc and abs(path_score(x, g, res.path) - want) <= 1e-12
            assert res.starts.tolist() == collapse_frames(res.path)[1]
            assert res.ends.tolist() == [s - 1 for s in res.starts.tolist()[1:]] + [4]


def test_align_host_raw_encoded_and_infeasible():
    rng = np.random.default_rng(3)
    x, g = rng.standard_normal((6, 4)), rng.standard_normal((4, 4))
    raw = [2, 2, 2, 3, 1, 1]
    assert encode_repeats(raw) == [2, 0, 2, 3, 1, 0]
    a = asg_viterbi_align_host(x, g, raw)
    b = asg_viterbi_align_host(x, g, encode_repeats(raw), encoded=True)
    assert a.feasible and a.path.tolist() == [2, 0, 2, 3, 1, 0] and a.starts.tolist() == list(range(6))
    assert a.score == b.score and a.path.tolist() == b.path.tolist() and a.ends.tolist() == b.ends.tolist()
    short = asg_viterbi_align_host(x[:2], g, [1, 2, 3])                     # S > T
    assert not short.feasible and short.score == -np.inf and short.path.tolist() == [-1, -1]
    assert short.starts.tolist() == [-1, -1, -1]
    assert not asg_viterbi_align_host(x, g, []).feasible
    with pytest.raises(ValueError, match='repeat label'):
        asg_viterbi_align_host(x, g, [1, 0, 2])
    with pytest.raises(ValueError, match='equal neighbours'):
        asg_viterbi_align_host(x, g, [1, 1], encoded=True)
    # float32 arithmetic on request, a tie goes to staying
    xt = np.zeros((3, 3), dtype=np.float32)
    tie = asg_viterbi_align_host(xt, np.zeros((3, 3), dtype=np.float32), [1, 2], encoded=True, dtype=np.float32)
    assert tie.score.dtype == np.float32 and tie.path.tolist() == [1, 2, 2]


def test_cli_values():
    from wav2letter_pytorch_amd import test as T
    base = ['model_path=a.ckpt', 'data.test_manifest=m.csv']
    asg = base + ['model.criterion=asg']
    with pytest.raises(SystemExit, match='criterion=asg'):
        T.build_config(base + ['decoder=asg_beam'])
    with pytest.raises(SystemExit, match='criterion=asg'):
        T.build_config(base + ['decoder=asg_beam_lm', 'lm_path=lm.arpa'])
    with pytest.raises(SystemExit, match='lm_path'):
        T.build_config(asg + ['decoder=asg_beam_lm'])
    with pytest.raises(SystemExit, match='lm_path'):
        T.build_config(asg + ['decoder=asg_beam', 'lm_path=lm.arpa'])
    cfg = T.build_config(asg + ['decoder=asg_beam', 'beam.k=7', 'beam.beta=2'])
    name, kw = T.decoder_spec(cfg, True)
    assert name == 'ASGBeamSearchDecoder' and kw['k'] == 7 and kw['beta'] == 2.0 and 'alpha' not in kw and 'log_probs' not in kw
    cfg = T.build_config(asg + ['decoder=asg_beam_lm', 'lm_path=lm.arpa', 'beam.alpha=0.7', 'beam.prune=1e-4'])
    name, kw = T.decoder_spec(cfg, True)
    assert name == 'ASGBeamSearchLMDecoder' and kw['lm_path'] == 'lm.arpa' and kw['alpha'] == 0.7 and kw['prune'] == 1e-4
    from wav2letter_pytorch_amd.asg import ASGDecoder
    from wav2letter_pytorch_amd.asg_beam import ASGBeamSearchDecoder, ASGBeamSearchLMDecoder
    dec = ASGBeamSearchLMDecoder(None, SMALL_LABELS, k=3)
    assert isinstance(dec, ASGBeamSearchDecoder) and isinstance(dec, ASGDecoder) and dec.lm is None and dec.k == 3


def test_abi_answers_on_the_host():
    from wav2letter_pytorch_amd._lib import lib
    assert lib.w2l_abi_version() == 2
    assert lib.w2l_asg_beam_search_workspace_bytes(2, 50, 65, 5, 0) == -1
    assert lib.w2l_asg_beam_search_workspace_bytes(2, 50, 29, 65, 0) == -1
    assert lib.w2l_asg_beam_search_workspace_bytes(2, 50, 29, 0, 0) == -1
    assert lib.w2l_asg_beam_search_workspace_bytes(2, 50, 29, 5, 0) > 0
    assert lib.w2l_asg_beam_search_workspace_bytes(1, 8, 64, 64, 0) > 0
    assert lib.w2l_asg_beam_search_workspace_bytes(2, 50, 29, 5, 7) == -1
    assert lib.w2l_asg_beam_search_workspace_bytes(2, 50, 29, 5, 3) > lib.w2l_asg_beam_search_workspace_bytes(2, 50, 29, 5, 0)
    assert lib.w2l_asg_align_workspace_bytes(2, 100, 29, 40) == 0
    assert lib.w2l_asg_align_workspace_bytes(2, 100, 65, 40) == -1 and lib.w2l_asg_align_workspace_bytes(2, 100, 29, 4096) == -1
    assert lib.w2l_asg_align_workspace_bytes(2, 32768, 29, 4095) > 0
