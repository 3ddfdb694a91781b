"""w2l_asg_align against asg_beam.asg_viterbi_align_host.

Bit-equality where fp32 arithmetic is exact: emissions and transitions that are multiples of 1/8 with |v| <= 16 and T <= 64
keep every partial sum a multiple of 1/8 below 2^11, so each fp32 add is exact and path, starts, ends and score must equal the
host's bit for bit, ties included.  One continuous case bounds the fp32 score by 2 T 2^-24 (sum of |terms| on the path): the
path's score is a chain of 2 T - 1 adds, each off by at most 2^-24 of a partial sum that the sum of |terms| bounds."""
import numpy as np
import pytest
import torch

from asg_beam_refs import log_softmax_scores, transitions
from wav2letter_pytorch_amd.asg import encode_repeats
from wav2letter_pytorch_amd.asg_beam import ASGBeamSearchDecoder, asg_beam_search_gpu, asg_forced_align, asg_viterbi_align_host
from wav2letter_pytorch_amd.data.label_sets import english_labels

pytestmark = pytest.mark.gpu


def _eighths(rng, shape, levels=129):
    """multiples of 1/8 in [-16, 16]; few ``levels`` make ties frequent"""
    return (rng.integers(0, levels, size=shape) * (256 // (levels - 1)) - 128).astype(np.float32) / 8


def _raw_target(rng, s, a, p_same=0.3):
    out = [int(rng.integers(1, a))]
    while len(out) < s:
        out.append(out[-1] if rng.random() < p_same else int(rng.integers(1, a)))
    return out


def _same(res, n, ref, t_n, s_n):
    assert bool(res.feasible[n]) == ref.feasible
    assert np.float32(res.scores[n]).tobytes() == np.float32(ref.score).tobytes(), (n, res.scores[n], ref.score)
    assert res.paths[n, :t_n].tolist() == ref.path.tolist() and (res.paths[n, t_n:] == -1).all()
    assert res.starts[n, :s_n].tolist() == ref.starts.tolist() and (res.starts[n, s_n:] == -1).all()
    assert res.ends[n, :s_n].tolist() == ref.ends.tolist() and (res.ends[n, s_n:] == -1).all()


@pytest.mark.parametrize('a,t,levels', [(3, 9, 3), (5, 33, 5), (29, 64, 129), (64, 40, 17)])
def test_bit_equal_where_fp32_is_exact(a, t, levels):
    rng = np.random.default_rng(a * 100 + t)
    n = 6
    x = _eighths(rng, (n, t, a), levels)
    g = _eighths(rng, (a, a), levels)
    lens = [t, t, t - 1, max(t // 2, 2), t, 3]
    slens = [1, min(t, 12), min(t - 1, 20), 2, t, 5]                     # S = 1, S = T, S > T (row 5: 5 labels, 3 frames)
    raws = [_raw_target(rng, s, a) for s in slens]
    raws[4] = _raw_target(rng, t, a, p_same=0.6)
    smax = max(slens)
    tg = np.zeros((n, smax), dtype=np.int32)
    for i, r in enumerate(raws):
        tg[i, :len(r)] = r
    res = asg_forced_align(x, g, tg, input_lengths=lens, target_lengths=slens)
    assert res.feasible.tolist() == [True] * 5 + [False]
    assert res.scores[5] == -np.inf and (res.paths[5] == -1).all() and (res.starts[5] == -1).all()
    for i in range(n):
        ref = asg_viterbi_align_host(x[i, :lens[i]], g, raws[i], dtype=np.float32)
        _same(res, i, ref, lens[i], slens[i])
        ref64 = asg_viterbi_align_host(x[i, :lens[i]], g, raws[i])
        assert float(ref64.score) == float(ref.score) and ref64.path.tolist() == ref.path.tolist()
    # the same rows already encoded, and a row with the repeat label in front
    enc = np.zeros_like(tg)
    for i, r in enumerate(raws):
        enc[i, :len(r)] = encode_repeats(r)
    res_e = asg_forced_align(x, g, enc, input_lengths=lens, target_lengths=slens, encoded=True)
    for f in ('scores', 'paths', 'starts', 'ends'):
        assert getattr(res_e, f).tobytes() == getattr(res, f).tobytes(), f
    lead = [0] + encode_repeats(raws[1])[:-1] if slens[1] > 1 else [0]
    got = asg_forced_align(x[1], g, [lead], encoded=True)
    _same(got, 0, asg_viterbi_align_host(x[1], g, lead, encoded=True, dtype=np.float32), t, len(lead))
    assert got.paths[0, 0] == 0 and got.starts[0, 0] == 0


@pytest.mark.parametrize('t,s', [(1000, 300), (1600, 1500), (2600, 2500)])
def test_larger_targets_take_the_other_kernel_shapes(t, s):
    """moves in 129 KB of LDS (512 threads); two and four states per thread with the moves in the workspace.  Multiples of 1/8
    in [-1/2, 1/2] keep the sums exact up to these T, so the device equals the host bit for bit"""
    rng = np.random.default_rng(t)
    a = 29
    x = (rng.integers(-4, 5, size=(2, t, a)) / 8).astype(np.float32)
    g = (rng.integers(-4, 5, size=(a, a)) / 8).astype(np.float32)
    raws = [_raw_target(rng, s, a), _raw_target(rng, s - 7, a)]
    tg = np.zeros((2, s), dtype=np.int32)
    for i, r in enumerate(raws):
        tg[i, :len(r)] = r
    lens, slens = [t, t - 5], [s, s - 7]
    res = asg_forced_align(x, g, tg, input_lengths=lens, target_lengths=slens)
    for i in range(2):
        _same(res, i, asg_viterbi_align_host(x[i, :lens[i]], g, raws[i], dtype=np.float32), lens[i], slens[i])


def test_continuous_inputs():
    t, s = 300, 40
    x = log_softmax_scores(77, (t, 29), scale=2.0)
    g = transitions(78, 29)
    raw = _raw_target(np.random.default_rng(79), s, 29)
    res = asg_forced_align(x, g, [raw])
    ref = asg_viterbi_align_host(x, g, raw)
    assert res.feasible[0] and ref.feasible
    assert res.paths[0].tolist() == ref.path.tolist()
    assert res.starts[0].tolist() == ref.starts.tolist() and res.ends[0].tolist() == ref.ends.tolist()
    p = ref.path
    terms = np.abs(x[np.arange(t), p].astype(np.float64)).sum() + np.abs(g[p[:-1], p[1:]].astype(np.float64)).sum()
    bound = 2 * t * 2.0 ** -24 * terms
    print(f'asg_align T={t} S={s}: score {res.scores[0]:.6f} ref {float(ref.score):.6f} '
          f'|diff| {abs(float(res.scores[0]) - float(ref.score)):.3e} bound {bound:.3e}')
    assert abs(float(res.scores[0]) - float(ref.score)) <= bound


def test_target_and_length_errors():
    x = log_softmax_scores(80, (2, 10, 29))
    g = transitions(81, 29)
    with pytest.raises(ValueError, match='repeat label'):
        asg_forced_align(x, g, [[1, 0, 2], [3]])
    with pytest.raises(ValueError, match='equal neighbours'):
        asg_forced_align(x, g, [[1, 1, 2], [3]], encoded=True)
    with pytest.raises(ValueError):
        asg_forced_align(x, g, [[1, 29], [3]])
    res = asg_forced_align(x, g, [[], [3]])                               # an empty target is infeasible, not an error
    assert res.feasible.tolist() == [False, True] and res.paths[1].tolist() == [3] * 10
    texts = asg_forced_align(x, g, ['HELLO', 'A B'], labels=english_labels)
    assert texts.feasible.all() and texts.target_lengths.tolist() == [5, 3]
    assert [english_labels[i] for i in texts.paths[0][texts.starts[0]]] == ['H', 'E', 'L', '_', 'O']


def test_decoder_offsets_equal_forced_alignment_of_the_text():
    from wav2letter_pytorch_amd.beam_search import get_time_per_word
    from asg_beam_refs import word_scores
    x = torch.from_numpy(word_scores(90, 3, 50, english_labels)).cuda()
    g = torch.from_numpy(transitions(91, 29, scale=0.3))
    sizes = torch.tensor([50, 37, 44])
    dec = ASGBeamSearchDecoder(english_labels, transitions=g, k=8, beta=1)
    texts, offsets = dec.decode(x, sizes, return_offsets=True)
    assert texts == dec.decode(x, sizes) and any(a == b for t in texts for a, b in zip(t, t[1:]))
    starts, ends = dec.align(x, texts, sizes=sizes)
    for n, text in enumerate(texts):
        assert len(text) > 0 and offsets[n][0].tolist() == starts[n][0].tolist()
        assert all(s <= e for s, e in zip(starts[n][0].tolist(), ends[n][0].tolist()))
        res = asg_forced_align(x[n], g, [text], input_lengths=[int(sizes[n])], labels=english_labels)
        assert res.starts[0, :len(text)].tolist() == offsets[n][0].tolist()
        words = get_time_per_word(text, starts[n][0].tolist(), 0.02, end_offsets=ends[n][0].tolist())
        assert [w for w, _, _ in words] == text.split()
    single = asg_beam_search_gpu(x[0], g, english_labels, k=8, beta=1, return_offsets=True)
    assert single[0] == texts[0] and single[1].tolist() == offsets[0][0].tolist()
