"""w2l_ctc_align (csrc/ctc_align.hip) against the host model it restates (alignment.viterbi_align_host in float32: the same
IEEE adds and compares in the same order, so every difference is a bug), and the decoders' ``return_offsets`` on top of it."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from wav2letter_pytorch_amd import _lib
from wav2letter_pytorch_amd.alignment import (align_sections, ctc_forced_align, launch_align, split_align,
                                              viterbi_align_host)
from wav2letter_pytorch_amd.beam_search import (GPUPrefixBeamSearchDecoder, GPUPrefixBeamSearchLMDecoder, get_time_per_word,
                                                prefix_beam_search_gpu)
from wav2letter_pytorch_amd.data.label_sets import english_labels
from wav2letter_pytorch_amd.decoder import GreedyDecoder

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def _log_probs(rng, n, t, a):
    """float32 log-softmax of random logits [n, t, a]"""
    z = rng.standard_normal((n, t, a)) * 2.0
    z -= z.max(-1, keepdims=True)
    return (z - np.log(np.exp(z).sum(-1, keepdims=True))).astype(np.float32)


def _targets(rng, n, a, lengths, blank=0, p_repeat=0.3):
    """random label rows with runs of repeated labels, padded to the longest"""
    rows = []
    for s in lengths:
        row = []
        while len(row) < s:
            if row and rng.random() < p_repeat:
                row.append(row[-1])
            else:
                c = int(rng.integers(0, a - 1))
                row.append(c + (c >= blank))
        rows.append(row)
    return rows


def _needed(row):
    return len(row) + sum(x == y for x, y in zip(row, row[1:]))


def _check_exact(lp, rows, res, input_lengths=None, blank=0):
    """every utterance: path, starts, ends equal and the score bit-equal to the float32 host model"""
    n, t, _ = lp.shape
    for u in range(n):
        tn = t if input_lengths is None else int(input_lengths[u])
        ref = viterbi_align_host(lp[u, :tn], rows[u], blank=blank, dtype=np.float32)
        s = len(rows[u])
        assert bool(res.feasible[u]) == ref.feasible, u
        assert np.float32(res.scores[u]).tobytes() == np.float32(ref.score).tobytes(), (u, res.scores[u], ref.score)
        assert np.array_equal(res.paths[u, :tn], ref.path), u
        assert (res.paths[u, tn:] == -1).all(), u
        assert np.array_equal(res.starts[u, :s], ref.starts), u
        assert np.array_equal(res.ends[u, :s], ref.ends), u
        assert (res.starts[u, s:] == -1).all() and (res.ends[u, s:] == -1).all(), u


# ------------------------------------------------------------------------------------------- exact agreement, log input
def test_exact_batch_ragged():
    """N = 32 x T = 500 x A = 29, ragged input lengths, targets of 0..150 labels with runs of repeats"""
    rng = np.random.default_rng(0)
    n, t, a = 32, 500, 29
    lp = _log_probs(rng, n, t, a)
    lengths = [0, 150, 1, 149] + [int(v) for v in rng.integers(0, 151, n - 4)]
    rows = _targets(rng, n, a, lengths)
    il = [int(v) for v in rng.integers(320, t + 1, n)]
    il[1] = t
    res = ctc_forced_align(lp, rows, input_lengths=il)
    assert res.feasible.all()
    _check_exact(lp, rows, res, il)


def test_exact_single_path():
    """T_n = S + repeats exactly: one path; one frame less: none"""
    rng = np.random.default_rng(1)
    n, t, a = 4, 64, 29
    lp = _log_probs(rng, n, t, a)
    rows = _targets(rng, n, a, [20, 31, 40, 12], p_repeat=0.4)
    il = [_needed(r) for r in rows]
    assert max(il) <= t
    res = ctc_forced_align(lp, rows, input_lengths=il)
    assert res.feasible.all()
    _check_exact(lp, rows, res, il)
    for u in range(n):                       # the single path has no blank but between repeats
        assert res.starts[u, :len(rows[u])].tolist() == res.ends[u, :len(rows[u])].tolist()
    il2 = [v - 1 for v in il]
    res = ctc_forced_align(lp, rows, input_lengths=il2)
    assert not res.feasible.any()
    _check_exact(lp, rows, res, il2)


def test_exact_one_utterance_and_2d_input():
    rng = np.random.default_rng(2)
    lp = _log_probs(rng, 1, 300, 29)
    rows = _targets(rng, 1, 29, [70])
    res = ctc_forced_align(lp, rows)
    _check_exact(lp, rows, res)
    res2 = ctc_forced_align(torch.from_numpy(lp[0]), rows[0], input_lengths=[250])
    _check_exact(lp, rows, res2, [250])


def test_exact_wide_alphabet_and_blank():
    """A = 128, and a non-zero blank"""
    rng = np.random.default_rng(3)
    n, t, a = 6, 200, 128
    lp = _log_probs(rng, n, t, a)
    rows = _targets(rng, n, a, [0, 5, 50, 99, 100, 64])
    _check_exact(lp, rows, ctc_forced_align(lp, rows))
    blank = 77
    rows = _targets(rng, n, a, [3, 0, 80, 99, 10, 64], blank=blank)
    _check_exact(lp, rows, ctc_forced_align(lp, rows, blank=blank), blank=blank)
    lp29 = _log_probs(rng, 3, 100, 29)
    rows = _targets(rng, 3, 29, [10, 30, 49], blank=28)
    _check_exact(lp29, rows, ctc_forced_align(lp29, rows, blank=28), blank=28)


def test_exact_strided_targets():
    """targets and lengths read with strides, as the beam search's device buffer holds them: rank 0 of [N, k, T] / [N, k]"""
    rng = np.random.default_rng(4)
    n, t, a, k, smax = 5, 120, 29, 3, 40
    lp = _log_probs(rng, n, t, a)
    rows = _targets(rng, n, a, [40, 0, 17, 33, 1])
    buf = rng.integers(1, a, (n, k, smax)).astype(np.int32)      # ranks 1.. hold other labels
    lens = rng.integers(0, smax, (n, k)).astype(np.int32)
    for u, r in enumerate(rows):
        buf[u, 0, :len(r)] = r
        lens[u, 0] = len(r)
    lens[1, 0] = -1                                               # an empty slot aligns as the empty target
    x = torch.from_numpy(lp).cuda()
    tg = torch.from_numpy(buf).cuda()
    tl = torch.from_numpy(lens).cuda()
    out = torch.empty(align_sections(n, t, smax)[5], dtype=torch.uint8, device='cuda')
    ws = launch_align(x, None, tg.data_ptr(), k * smax, tl.data_ptr(), k, smax, 0, True, out, 0)
    scores, status, paths, starts, ends = split_align(out.cpu().numpy(), n, t, smax)
    del ws
    assert not status.any()

    class R:
        pass
    res = R()
    res.scores, res.feasible, res.paths, res.starts, res.ends = scores, status == 0, paths, starts, ends
    _check_exact(lp, rows, res)


def test_exact_long():
    """T = 8 000 frames with S = 4 000 labels (the limits w2l_ctc_loss is tested at): 8 001 states, 8 per thread, the
    back-pointers in the workspace"""
    rng = np.random.default_rng(5)
    n, t, a = 2, 8000, 29
    lp = _log_probs(rng, n, t, a)
    rows = _targets(rng, n, a, [4000, 2500], p_repeat=0.2)
    assert _lib.lib.w2l_ctc_align_workspace_bytes(n, t, 4000) > 0
    res = ctc_forced_align(lp, rows)
    assert res.feasible.all()
    _check_exact(lp, rows, res)


def test_exact_mid_shapes():
    """every block shape of the launch: 64 .. 1024 threads, 2 and 4 states per thread"""
    rng = np.random.default_rng(6)
    for s, t in [(20, 100), (60, 200), (120, 300), (250, 600), (500, 1100), (1000, 2100), (2000, 4100)]:
        lp = _log_probs(rng, 2, t, 29)
        rows = _targets(rng, 2, 29, [s, s // 2])
        _check_exact(lp, rows, ctc_forced_align(lp, rows, input_lengths=[t, t - 7]), [t, t - 7])


def test_limits_are_errors():
    assert _lib.lib.w2l_ctc_align_workspace_bytes(1, 100, 4096) == -1
    assert _lib.lib.w2l_ctc_align_workspace_bytes(1, 32769, 10) == -1
    assert _lib.lib.w2l_ctc_align_workspace_bytes(4, 500, 150) == 0
    x = torch.zeros(1, 8, 4, device='cuda')
    out = torch.empty(align_sections(1, 8, 4096)[5], dtype=torch.uint8, device='cuda')
    tg = torch.ones(4097, dtype=torch.int32, device='cuda')
    vp = C.c_void_p
    rc = _lib.lib.w2l_ctc_align(vp(x.data_ptr()), None, vp(tg.data_ptr()), 4096, vp(tg.data_ptr()), 1, 1, 8, 4, 4096, 0, 1, None,
                                0, vp(out.data_ptr()), vp(out.data_ptr()), vp(out.data_ptr()), vp(out.data_ptr()),
                                vp(out.data_ptr()), _lib.stream_ptr())
    assert rc != 0 and b'out of range' in _lib.lib.w2l_last_error()


# ------------------------------------------------------------------------------------------------- probability input
def test_probability_input_with_zeros():
    """log_probs=False on float32 probabilities with exact zeros: the path collapses to the target, and its score, re-summed
    on the host in float64, is within tol of the float64 optimum.  tol is derived: the kernel's score is a chain of T fp32
    adds, each rounding by at most 2**-24 of the partial sum (|partial| <= M), and so is the score of any rival path it
    compares with: 2 * T * 2**-24 * M; logf of each emission is good to 2 ulp of |lp| at most: T * 2**-22 * max|lp|."""
    rng = np.random.default_rng(7)
    n, t, a = 8, 300, 29
    p = np.exp(_log_probs(rng, n, t, a)).astype(np.float32)
    p[rng.random(p.shape) < 0.2] = 0.0
    p[:, :, 0] = np.maximum(p[:, :, 0], 1e-3)              # the blank stays possible
    rows = _targets(rng, n, a, [int(v) for v in rng.integers(0, 40, n)])
    for u, r in enumerate(rows):                            # and one frame in four carries each target label
        for j, c in enumerate(r):
            p[u, j::4, c] = np.maximum(p[u, j::4, c], 1e-2)
    res = ctc_forced_align(p, rows, log_probs=False)
    with np.errstate(divide='ignore'):
        lp = np.log(p.astype(np.float64))
    for u in range(n):
        ref = viterbi_align_host(lp[u], rows[u])
        assert ref.feasible and res.feasible[u]
        path = res.paths[u]
        prev = np.concatenate(([-1], path[:-1]))
        assert path[(path != prev) & (path != 0)].tolist() == rows[u], u
        resum = lp[u][np.arange(t), path].sum()
        finite = lp[u][np.isfinite(lp[u])]
        m = abs(ref.score) + np.abs(finite).max()
        tol = 2 * t * 2.0 ** -24 * m + t * 2.0 ** -22 * np.abs(finite).max()
        print('utterance %d: resummed %.9f optimum %.9f diff %.3e tol %.3e' % (u, resum, ref.score, ref.score - resum, tol))
        assert np.isfinite(resum) and abs(resum - ref.score) <= tol, (u, resum, ref.score, tol)
        assert abs(float(res.scores[u]) - ref.score) <= tol, (u, res.scores[u], ref.score, tol)


# ---------------------------------------------------------------------------------------------------------------- status
def test_status_infeasible_beside_feasible():
    rng = np.random.default_rng(8)
    n, t, a = 6, 40, 29
    lp = _log_probs(rng, n, t, a)
    rows = _targets(rng, n, a, [10, 39, 5, 30, 0, 20], p_repeat=0.5)
    il = [40, 40, 4, 40, 1, 40]                            # utterance 2: 5 labels on 4 frames
    p = np.exp(lp)
    p[5, 7, :] = 0.0                                       # utterance 5: a frame no label can pass
    lp[5, 7, :] = -np.inf
    for probs, flag in ((lp, True), (p, False)):
        res = ctc_forced_align(probs, rows, input_lengths=il, log_probs=flag)
        want = [_needed(r) <= tn for r, tn in zip(rows, il)]
        want[5] = False
        assert res.feasible.tolist() == want
        assert not want[2] and want[0] and want[4]
        for u in range(n):
            if not want[u]:
                assert res.scores[u] == -np.inf
                assert (res.paths[u] == -1).all() and (res.starts[u] == -1).all() and (res.ends[u] == -1).all()
        if flag:
            _check_exact(lp, rows, res, il)


def test_status_errors_raise():
    rng = np.random.default_rng(9)
    lp = _log_probs(rng, 3, 30, 29)
    rows = _targets(rng, 3, 29, [5, 6, 7])
    p = np.exp(lp)
    p[1, 29, 28] = -1e-3                                   # a label the target does not even hold
    with pytest.raises(ValueError, match=r'utterances \[1\]'):
        ctc_forced_align(p, rows, log_probs=False)
    p[1, 29, 28] = np.nan
    with pytest.raises(ValueError, match=r'utterances \[1\]'):
        ctc_forced_align(p, rows, log_probs=False)
    bad = [list(r) for r in rows]
    bad[2][3] = 29
    with pytest.raises(ValueError, match=r'utterances \[2\]'):
        ctc_forced_align(lp, bad)
    bad[2][3] = 0
    with pytest.raises(ValueError, match=r'utterances \[2\]'):
        ctc_forced_align(lp, bad)
    bad[2][3] = -5
    bad[0][0] = 1 << 20
    with pytest.raises(ValueError, match=r'utterances \[0, 2\]'):
        ctc_forced_align(lp, bad)
    ctc_forced_align(lp, rows)                             # the device is fine afterwards


# ------------------------------------------------------------------------------------------------- the reference's fixture
def test_greedy_fixture_through_the_device():
    """tests/golden/greedy_cases.npz: starts == the reference GreedyDecoder's offsets for utterances 0, 1 and 3; utterance 2
    holds an exactly uniform frame (frame 5; argmax takes the lowest index, Viterbi need not): the score equals the argmax
    path's and the path collapses to the string"""
    z = np.load(os.path.join(GOLD, 'greedy_cases.npz'), allow_pickle=True)
    labels = list(z['labels'])
    sizes = [int(v) for v in z['sizes']]
    strings = [str(s) for s in z['strings']]
    res = ctc_forced_align(z['probs'], strings, input_lengths=sizes, log_probs=False, labels=labels)
    assert res.feasible.all()
    first = {}
    for i, ch in enumerate(labels):
        first.setdefault(ch, i)
    for n in range(4):
        path = res.paths[n, :sizes[n]]
        prev = np.concatenate(([-1], path[:-1]))
        assert path[(path != prev) & (path != 0)].tolist() == [first[ch] for ch in strings[n]]
        if n == 2:
            with np.errstate(divide='ignore'):
                lp = np.log(z['probs'][n, :sizes[n]].astype(np.float64))
            ref = lp[np.arange(sizes[n]), z['argmax'][n, :sizes[n]]].sum()
            tol = 2 * sizes[n] * 2.0 ** -24 * abs(ref) + sizes[n] * 2.0 ** -22 * np.abs(lp[np.isfinite(lp)]).max()
            assert abs(float(res.scores[n]) - ref) <= tol
        else:
            assert res.starts[n, :len(strings[n])].tolist() == list(z['offsets'][n]), n
    dec = GreedyDecoder(labels, blank_index=0)
    offsets, end_offsets = dec.align(torch.from_numpy(z['probs']), strings, sizes)
    for n in (0, 1, 3):
        assert offsets[n][0].dtype == torch.int32 and offsets[n][0].tolist() == list(z['offsets'][n])
        assert all(e >= s for s, e in zip(offsets[n][0].tolist(), end_offsets[n][0].tolist()))


# --------------------------------------------------------------------------------------------------------------- decoders
def _peaky(seed, n, t, a, blank=0, boost=(5.0, 11.0), p_blank=0.6, max_burst=3):
    """tests/test_gpu_beam_search.py's generator restated: blank-dominant synthetic posteriors with bursts of one character,
    float32 [n, t, a]; each blank frame or burst lifts its label's logit by a boost drawn from the range ``boost``"""
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


def _check_decoder_offsets(dec, p, sizes):
    labels = list(dec.labels)
    first = {}
    for i, ch in enumerate(labels):
        first.setdefault(ch, i)
    x = torch.from_numpy(p).cuda()
    sz = None if sizes is None else torch.tensor(sizes)
    plain = dec.decode(x, sz)
    strings, offsets = dec.decode(x, sz, return_offsets=True)
    assert strings == plain
    assert len(offsets) == len(strings)
    with np.errstate(divide='ignore'):
        lp = np.log(p)                                     # float32, the kernel's logf up to its rounding
    for n, s in enumerate(strings):
        tn = p.shape[1] if sizes is None else sizes[n]
        assert isinstance(offsets[n], list) and len(offsets[n]) == 1
        off = offsets[n][0]
        assert off.dtype == torch.int32 and off.dim() == 1 and off.numel() == len(s)
        ref = viterbi_align_host(lp[n, :tn], [first[ch] for ch in s], dtype=np.float32)
        assert ref.feasible
        assert off.tolist() == ref.starts.tolist(), (n, s)
        words = get_time_per_word(s, off, 0.02)
        assert [w for w, _, _ in words] == s.split()
    return strings


@pytest.mark.parametrize('k', [5, 16])
@pytest.mark.parametrize('with_sizes', [False, True])
def test_beam_decoder_offsets(k, with_sizes):
    p = _peaky(11 + k, 8, 200, len(english_labels))
    sizes = [200, 150, 199, 2, 57, 200, 101, 180] if with_sizes else None
    dec = GPUPrefixBeamSearchDecoder(None, english_labels, k=k)
    strings = _check_decoder_offsets(dec, p, sizes)
    assert any(' ' in s for s in strings)
    # one utterance, 2-D
    s1, o1 = dec.decode(torch.from_numpy(p[0]).cuda(), return_offsets=True)
    s_all, o_all = dec.decode(torch.from_numpy(p).cuda(), return_offsets=True)
    assert s1 == s_all[0] and len(o1) == 1 and o1[0].tolist() == o_all[0][0].tolist()
    with pytest.raises(ValueError, match='nbest'):
        prefix_beam_search_gpu(p, english_labels, k=k, nbest=2, return_offsets=True)


def _write_arpa(path):
    words = ['A', 'B', 'AB', 'BA', 'CAB', 'E', 'DE', 'ED']
    uni = ['-2.0\t<unk>', '-99\t<s>\t-0.3', '-1.0\t</s>\t0'] + ['%.2f\t%s\t%.2f' % (-0.5 - 0.1 * i, w, -0.2 - 0.05 * i)
                                                                  for i, w in enumerate(words)]
    bi = ['%.2f\t%s %s' % (-0.3 - 0.07 * ((3 * i + j) % 7), a, b) for i, a in enumerate(['<s>'] + words)
          for j, b in enumerate(words + ['</s>']) if (i + j) % 3 != 1]
    text = '\\data\\\nngram 1=%d\nngram 2=%d\n\n\\1-grams:\n%s\n\n\\2-grams:\n%s\n\n\\end\\\n' % (len(uni), len(bi), '\n'.join(uni),
                                                                                                     '\n'.join(bi))
    path.write_text(text)
    return str(path)


@pytest.mark.parametrize('k', [5, 16])
@pytest.mark.parametrize('with_sizes', [False, True])
def test_lm_decoder_offsets(tmp_path, k, with_sizes):
    rng = np.random.default_rng(40 + k)
    a = len(english_labels)
    p = _peaky(21 + k, 8, 200, a)
    # favour the LM's letters and the space, so that words close and the model is consulted
    keep = [0] + [english_labels.index(c) for c in 'ABCDE '] + [int(v) for v in rng.integers(1, a, 2)]
    w = np.full(a, 0.02, dtype=np.float32)
    w[keep] = 1.0
    p = p * w
    p = (p / p.sum(-1, keepdims=True)).astype(np.float32)
    sizes = [200, 150, 199, 2, 57, 200, 101, 180] if with_sizes else None
    dec = GPUPrefixBeamSearchLMDecoder(_write_arpa(tmp_path / 'm.arpa'), english_labels, k=k, alpha=1.0, beta=2)
    _check_decoder_offsets(dec, p, sizes)


def test_empty_decode_gives_empty_offsets():
    a = len(english_labels)
    p = np.full((3, 20, a), 1e-4, dtype=np.float32)
    p[:, :, 0] = 1.0
    p[1, 5:8, 3] = 50.0
    p /= p.sum(-1, keepdims=True)
    dec = GPUPrefixBeamSearchDecoder(None, english_labels, k=5)
    strings, offsets = dec.decode(torch.from_numpy(p).cuda(), return_offsets=True)
    assert strings == ['', 'B', '']
    assert offsets[0][0].dtype == torch.int32 and offsets[0][0].numel() == 0 and offsets[2][0].numel() == 0
    assert offsets[1][0].tolist() == [5]
    assert get_time_per_word(strings[0], offsets[0][0]) == []
    assert get_time_per_word(strings[1], offsets[1][0], 0.5) == [('B', 2.5, 2.5)]


def test_greedy_offsets_equal_align_of_its_strings():
    """blank-dominant posteriors with unique frame maxima: the argmax path is the best path of the string it collapses to"""
    p = _peaky(31, 8, 200, len(english_labels))
    top = np.sort(p, -1)
    assert (top[:, :, -1] > top[:, :, -2]).all()
    dec = GreedyDecoder(english_labels, blank_index=0)
    sizes = torch.tensor([200, 150, 199, 1, 57, 200, 101, 180])
    x = torch.from_numpy(p).cuda()
    strings, offsets = dec.decode(x, sizes, return_offsets=True)
    got, got_ends = dec.align(x, strings, sizes)
    for n in range(8):
        assert got[n][0].dtype == offsets[n][0].dtype == torch.int32
        assert got[n][0].tolist() == offsets[n][0].tolist(), n
        assert get_time_per_word(strings[n], got[n][0], 1.0, end_offsets=got_ends[n][0]) is not None
        assert all(e >= s for s, e in zip(got[n][0].tolist(), got_ends[n][0].tolist()))
    with pytest.raises(ValueError, match='no frame path'):
        dec.align(x[:1, :3], ['ABCD'])


# ------------------------------------------------------------------------------------------------------------ launch trace
def test_trace_shows_one_align_row_only_with_offsets(tmp_path):
    p = torch.from_numpy(_peaky(5, 4, 100, len(english_labels))).cuda()
    dec = GPUPrefixBeamSearchDecoder(None, english_labels, k=5)
    dec.decode(p, return_offsets=True)                     # warm-up outside the trace

    def rows(fn):
        torch.cuda.synchronize()
        _lib.trace_launches(True)
        try:
            fn()
            torch.cuda.synchronize()
        finally:
            _lib.trace_launches(False)
        path = tmp_path / 'trace.csv'
        n = _lib.trace_dump(str(path))
        names = [line.split(',')[0] for line in path.read_text().splitlines()[1:]] if n else []
        return names

    names = rows(lambda: dec.decode(p, return_offsets=True))
    assert names.count('ctc_beam_search_kernel') == 1 and names.count('ctc_align_kernel') == 1
    assert names.index('ctc_beam_search_kernel') < names.index('ctc_align_kernel')
    names = rows(lambda: dec.decode(p))
    assert names.count('ctc_beam_search_kernel') == 1 and 'ctc_align_kernel' not in names
