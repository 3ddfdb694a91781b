"""w2l_asg_loss and w2l_asg_viterbi (csrc/asg.hip) called directly on a real MI355X against the float64 reference with derived
per-element bounds (asg_refs.asg_ref, pinned by tests/test_cpu_asg.py): ratio = max |got - ref| / bound <= 1 over the loss, every
nll, EVERY element of d loss / d x and EVERY element of d loss / d transitions.  Every buffer, the workspace included, starts as
NaN (a bit pattern for integers), is sized exactly at the query and is followed by a guard region that is checked after every call.

Which case reaches which kernel (asg_chains_kernel<AP, NT, SPT>; every case prints its own; both reductions each):

  A1 A5 A32 A33 A64      T 12, mixed lengths            AP 32 and 64, a wave with and without -inf padding lanes; <*, 64, 1>
  S64 .. S1024           A 5, Smax at both edges of     <32, 64 | 128 | 256 | 512 | 1024, 1>; S = Smax in T = S + 6 frames beside a
                         every block width              short, an infeasible (status 1) and an empty utterance in one launch
  S1025 S2048            A 5, S = Smax                  <32, 1024, 2>: two states per thread, all slots live
  S2049 S3073 S4095      A 5, S = Smax                  <32, 1024, 4>: spt 3 rounded up to 4, and 4; 2 frames per posterior pass
  A64-S4095              T 70, S 20 and 9               <64, 1024, 4>; asg_grad_kernel with 115 KB of dynamic LDS; two frame chunks
  A64-S513               T 130, S 100 and 40            <64, 1024, 1>; three chunks, the slab sum over N * 3
  A33-S100 .. A33-S1500  T 12, padded Smax              <64, 128 | 256 | 512, 1> and <64, 1024, 2>
  T64 T65 T128 T129      in_len T, 64, 63, 1, 0         chunk edges, blocks with t0 >= Tn, Tn = 0, rows past Tn
  fb127 fb128 fb129      T 140, S = Smax                64 / 64 / 63 frames per pass of the target-posterior buffer: one pass, two
  runs                   runs of 2, 3, 4, 5 and 24      the encoding's backward scan (the long transcripts hold a run of four across
                                                        every thread-count boundary 64 .. 3072)
  bad-*                  a label < 0, = A, = repeat     status 2 contributes nothing; repeat index 0 and A - 1
  clamps                 tg_len > Smax, in_len > T, < 0

Then the refusals (nothing written), and the Viterbi decoder on small integers, where every score is exact in fp32 and every tie
must fall as documented: the lowest predecessor, the lowest final label."""
import numpy as np
import pytest
import torch

import asg_refs as R
from direct_helpers import Buf, guards, last_error, p, ratio, record
from frontend_refs import split_nonfinite

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def L():
    from wav2letter_pytorch_amd import _lib
    assert torch.cuda.is_available()
    return _lib


def up(a, dtype=torch.float32):
    return Buf(a.shape, dtype, torch.from_numpy(np.ascontiguousarray(a)))


def run(L, rc):
    """check the launch and wait for it; a HIP error ends the session: nothing more is launched on a device that has faulted"""
    try:
        L.check(rc)
        torch.cuda.synchronize()
    except Exception as e:                              # noqa: BLE001
        pytest.exit(f'HIP error in a direct asg launch, nothing more is run: {e}', returncode=3)


def bounded(case, got, ref, bound):
    ok, g, r = split_nonfinite(got, ref)
    assert ok, f'{case}: inf / NaN pattern differs from the reference'
    return record('asg', case, ratio(g, r, np.where(np.isfinite(bound), bound, 0.0)))


class Inputs:
    def __init__(self, c):
        self.x, self.g = up(c.x), up(c.g)
        self.tg, self.il, self.tl = up(c.targets, torch.int32), up(c.in_len, torch.int32), up(c.tg_len, torch.int32)

    def all(self):
        return self.x, self.g, self.tg, self.il, self.tl


def asg_run(L, c, reduction, inp, grads=True):
    N, T, A = c.dims
    nll, loss, status = Buf((N,)), Buf((1,)), Buf((N,), torch.int32)
    gx = Buf((N, T, A)) if grads else None
    gg = Buf((A, A)) if grads else None
    nbytes = L.lib.w2l_asg_workspace_bytes(N, T, A, c.Smax)
    assert nbytes == R.asg_workspace_bytes(N, T, A, c.Smax)
    ws = Buf((nbytes // 4,))
    run(L, L.lib.w2l_asg_loss(p(L, inp.x), p(L, inp.g), p(L, inp.tg), p(L, inp.il), p(L, inp.tl), N, T, A, c.Smax, c.repeat,
                              {'mean': 0, 'sum': 1}[reduction], p(L, nll), p(L, loss), p(L, gx), p(L, gg), p(L, status), p(L, ws),
                              nbytes, L.stream_ptr()))
    assert guards(*inp.all(), nll, loss, status, gx, gg, ws), f'{c.name}: a guard region was written'
    return dict(nll=nll.np(), loss=loss.np(), status=status.np(), grad_x=None if gx is None else gx.np(),
                grad_g=None if gg is None else gg.np())


@pytest.mark.parametrize('reduction', ['mean', 'sum'])
@pytest.mark.parametrize('name', list(R.CASES))
def test_asg_loss_and_gradients_per_element(L, name, reduction):
    c = R.case(name)
    r = R.case_ref(name, reduction)
    tag = f'{name}/{reduction}'
    print(tag, 'dims', c.dims, 'Smax', c.Smax, 'variant (AP, NT, SPT, grad LDS bytes):', c.variant)
    inp = Inputs(c)
    got = asg_run(L, c, reduction, inp)
    assert got['status'].tolist() == r['status'].tolist(), tag
    rs = [bounded(tag + '-nll', got['nll'], r['nll'], r['nll_b']),
          bounded(tag + '-loss', got['loss'], np.array([r['loss']]), np.array([r['loss_b']])),
          bounded(tag + '-grad_x', got['grad_x'], r['grad_x'], r['grad_x_b']),
          bounded(tag + '-grad_g', got['grad_g'], r['grad_g'], r['grad_g_b'])]
    assert max(rs) <= 1.0, (tag, rs)
    gx = got['grad_x'].astype(np.float64)
    for n in range(c.dims[0]):
        assert not gx[n, r['Tn'][n]:].any(), 'gradient rows past the input length must be exactly 0'
        if r['status'][n]:
            assert got['nll'][n] == 0.0 and not gx[n].any(), 'an infeasible or bad utterance contributes nothing'
    # both posteriors sum to 1 over the labels: a row of the reference sums to 0, a device row to at most the sum of its bounds
    assert (np.abs(gx.sum(axis=2)) <= r['grad_x_b'].sum(axis=2) + 1e-300).all(), tag
    # the loss alone is the same number, and a second call gives the same bits
    alone = asg_run(L, c, reduction, inp, grads=False)
    assert np.array_equal(alone['loss'], got['loss']) and np.array_equal(alone['nll'], got['nll'])
    assert alone['status'].tolist() == got['status'].tolist()
    again = asg_run(L, c, reduction, inp)
    for k in ('loss', 'nll', 'grad_x', 'grad_g'):
        assert np.array_equal(again[k], got[k]), (tag, k)


def test_bad_labels_leave_their_neighbours_alone(L):
    """the two good utterances of a bad-label case give the nll they give without the bad one between them"""
    c = R.case('bad-A-r5')
    got = asg_run(L, c, 'sum', Inputs(c))
    keep = [0, 2]
    d = R.AsgCase('bad-A-r5-good', c.x[keep], c.g, c.targets[keep], c.in_len[keep], c.tg_len[keep], c.Smax, c.repeat)
    good = asg_run(L, d, 'sum', Inputs(d))
    assert got['status'].tolist() == [0, 2, 0] and good['status'].tolist() == [0, 0]
    assert np.array_equal(got['nll'][keep], good['nll']) and np.array_equal(got['grad_x'][keep], good['grad_x'])
    assert np.array_equal(got['grad_g'], good['grad_g']) and got['loss'][0] == good['loss'][0]


def test_rejected_arguments_write_nothing(L):
    c = R.case('A5')
    N, T, A = c.dims
    inp = Inputs(c)
    nll, loss, status, gx, gg = Buf((N,)), Buf((1,)), Buf((N,), torch.int32), Buf((N, T, A)), Buf((A, A))
    nbytes = L.lib.w2l_asg_workspace_bytes(N, T, A, c.Smax)
    ws = Buf((nbytes // 4,))

    def call(A_=A, Smax=c.Smax, repeat=0, reduction=0, gx_=gx, gg_=gg, nb=nbytes):
        rc = L.lib.w2l_asg_loss(p(L, inp.x), p(L, inp.g), p(L, inp.tg), p(L, inp.il), p(L, inp.tl), N, T, A_, Smax, repeat, reduction,
                                p(L, nll), p(L, loss), p(L, gx_), p(L, gg_), p(L, status), p(L, ws), nb, L.stream_ptr())
        torch.cuda.synchronize()
        return rc, last_error(L)

    for kw, word in ((dict(nb=nbytes - 1), 'workspace'), (dict(gg_=None), 'go together'), (dict(repeat=A), 'repeat_index'),
                     (dict(reduction=2), 'reduction'), (dict(A_=65), 'out of range'), (dict(Smax=4096), 'out of range')):
        rc, msg = call(**kw)
        assert rc != 0 and word in msg, (kw, rc, msg)
    assert guards(*inp.all(), nll, loss, status, gx, gg, ws)
    for b in (nll, loss, gx, gg, ws):
        assert torch.isnan(b.t).all()
    assert (status.t == status.pattern).all()


@pytest.mark.parametrize('T', R.VITERBI_T)
@pytest.mark.parametrize('A', R.VITERBI_A)
def test_viterbi_is_exact_on_integers_ties_included(L, A, T):
    x, g, in_len, refs, refs_full = R.viterbi_case(A, T)
    if A > 1:                                           # the reference itself rests on ties here
        assert refs[0][2] == 0.0 and refs_full[1][2] == 0.0 and refs[2][2] == 0.0
    N = x.shape[0]
    xd, gd, ild = up(x), up(g), up(in_len, torch.int32)
    nbytes = L.lib.w2l_asg_viterbi_workspace_bytes(N, T, A)
    assert nbytes == N * T * (32 if A <= 32 else 64)
    for lens, want in ((None, refs_full), (ild, refs)):
        path, score, ws = Buf((N, T), torch.int32), Buf((N,)), Buf((nbytes,), torch.uint8)
        run(L, L.lib.w2l_asg_viterbi(p(L, xd), p(L, gd), p(L, lens), N, T, A, p(L, ws), nbytes, p(L, path), p(L, score),
                                     L.stream_ptr()))
        assert guards(xd, gd, ild, path, score, ws), 'a guard region was written'
        got, sc = path.np(), score.np()
        for n in range(N):
            tn = len(want[n][0])
            assert got[n, :tn].tolist() == want[n][0], (A, T, n, 'in_len' if lens is not None else 'NULL')
            assert (got[n, tn:] == -1).all()
            assert sc[n] == np.float32(want[n][1]) and float(sc[n]) == want[n][1], (A, T, n)
    rc = L.lib.w2l_asg_viterbi(p(L, xd), p(L, gd), p(L, ild), N, T, A, p(L, ws), nbytes - 1, p(L, path), p(L, score), L.stream_ptr())
    assert rc != 0 and 'workspace' in last_error(L)
