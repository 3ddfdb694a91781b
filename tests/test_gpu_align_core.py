"""The instantiations csrc/align_core.h's launcher picks that tests/test_gpu_ctc_align.py and tests/test_gpu_asg_align.py do
not reach bit for bit: every case here names the block shape (threads x states per thread) and where the moves live, checks
both through the workspace query, and compares the launch with the float32 host model (viterbi_align_host,
asg_viterbi_align_host).  Scores are integers of magnitude <= 64, so with T <= 600 every float32 sum is an integer below 2^24
and exact: path, starts, ends and score must equal the host's bit for bit, ties (frequent with integers) included.

The block shape follows Smax, the width of the padded target array, not the rows' own lengths; that is how the wide shapes run
with their moves in LDS, which only a short T allows: short rows in a wide array.  Shapes: N = 2, the second row with fewer
frames and labels, A = 5, S just above the step of the shape, T = S + 8 (CTC: plus the adjacent repeats)."""
import numpy as np
import pytest

from wav2letter_pytorch_amd import _lib
from wav2letter_pytorch_amd.alignment import ctc_forced_align, viterbi_align_host
from wav2letter_pytorch_amd.asg_beam import asg_forced_align, asg_viterbi_align_host

pytestmark = pytest.mark.gpu
A = 5


def _rows(rng, lengths, p_same=0.3):
    """label rows over 1 .. A-1 (0 is the blank / the repeat label) with runs of equal labels"""
    rows = []
    for s in lengths:
        row = [int(rng.integers(1, A))]
        while len(row) < s:
            row.append(row[-1] if rng.random() < p_same else int(rng.integers(1, A)))
        rows.append(row)
    return rows


def _padded(rows, smax):
    tg = np.zeros((len(rows), smax), dtype=np.int32)
    for i, r in enumerate(rows):
        tg[i, :len(r)] = r
    return tg


def _plan(query, n, t, smax):
    """(states of the block = threads x states per thread, whether the moves live in LDS) as the workspace query gives them
    away: beyond LDS it answers N x chunks x states x 4 bytes, and T = 32768 (2048 chunks) is beyond LDS for every shape"""
    return query(1, 32768, smax) // (2048 * 4), query(n, t, smax) == 0


def _same(res, u, ref, t_n, s_n):
    assert bool(res.feasible[u]) == ref.feasible and ref.feasible
    assert np.float32(res.scores[u]).tobytes() == np.float32(ref.score).tobytes(), (u, res.scores[u], ref.score)
    assert res.paths[u, :t_n].tolist() == ref.path.tolist() and (res.paths[u, t_n:] == -1).all()
    assert res.starts[u, :s_n].tolist() == ref.starts.tolist() and (res.starts[u, s_n:] == -1).all()
    assert res.ends[u, :s_n].tolist() == ref.ends.tolist() and (res.ends[u, s_n:] == -1).all()


# Smax, the rows' lengths, states of the block, moves in LDS.  2 Smax + 1 states: 513 -> 1024 x 1, 1025 -> 1024 x 2,
# 2049 -> 1024 x 4, 4097 -> 1024 x 8 (whose moves fit LDS up to T = 32)
@pytest.mark.parametrize('smax,lengths,states,in_lds', [(256, [256, 100], 1024, True), (512, [40, 17], 2048, True),
                                                        (1024, [40, 17], 4096, True), (2048, [12, 5], 8192, True)])
def test_ctc_shapes_with_moves_in_lds(smax, lengths, states, in_lds):
    rng = np.random.default_rng(smax)
    rows = _rows(rng, lengths)
    t = lengths[0] + 8 + sum(x == y for x, y in zip(rows[0], rows[0][1:]))
    lens = [t, t - 3]
    assert _plan(_lib.lib.w2l_ctc_align_workspace_bytes, 2, t, smax) == (states, in_lds)
    lp = rng.integers(-64, 65, size=(2, t, A)).astype(np.float32)
    res = ctc_forced_align(lp, _padded(rows, smax), input_lengths=lens, target_lengths=lengths)
    for u in range(2):
        _same(res, u, viterbi_align_host(lp[u, :lens[u]], rows[u], dtype=np.float32), lens[u], lengths[u])


# 65 states -> 128 x 1, 129 -> 256 x 1, 513 -> 1024 x 1 (in LDS up to T = 560), 1025 -> 1024 x 2, 2049 -> 1024 x 4
@pytest.mark.parametrize('smax,lengths,t,states,in_lds', [(65, [65, 30], 73, 128, True), (129, [129, 60], 137, 256, True),
                                                          (513, [513, 200], 521, 1024, True),
                                                          (513, [513, 200], 600, 1024, False),
                                                          (1025, [40, 17], 48, 2048, True), (2049, [40, 17], 48, 4096, True)])
def test_asg_shapes(smax, lengths, t, states, in_lds):
    rng = np.random.default_rng(smax + t)
    rows = _rows(rng, lengths)
    lens = [t, t - 3]
    assert _plan(lambda n, t_, s: _lib.lib.w2l_asg_align_workspace_bytes(n, t_, A, s), 2, t, smax) == (states, in_lds)
    x = rng.integers(-64, 65, size=(2, t, A)).astype(np.float32)
    g = rng.integers(-64, 65, size=(A, A)).astype(np.float32)
    res = asg_forced_align(x, g, _padded(rows, smax), input_lengths=lens, target_lengths=lengths)
    for u in range(2):
        _same(res, u, asg_viterbi_align_host(x[u, :lens[u]], g, rows[u], dtype=np.float32), lens[u], lengths[u])
