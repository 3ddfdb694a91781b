"""w2l_wctc_loss (csrc/wctc.hip) called directly on a real MI355X against its float64 reference (tests/wctc_refs.py, itself pinned
by tests/test_cpu_wctc.py) under the derived per-element bound: ratio = max |got - ref| / bound <= 1 over the loss, every nll and
EVERY gradient element.  Outputs start as NaN and are followed by a guard region that is checked after every call.

Which case reaches which kernel (C = 29, N = 3, unequal input lengths, one below T):

  L63    Smax 31,  T 56     ctc_alpha_beta_kernel<WctcParams, 64, 1, staged> (csrc/ctc_core.h)
  L65    Smax 32,  T 80     <128, 1, staged>
  L129   Smax 64,  T 160    <192, 1, staged>
  L1025  Smax 512, T 600    <1024, 2, staged>: two states per thread; rows longer than one 256-entry chunk of the parse kernel
  mem    Smax 8,   T 1400   <64, 1, from memory>: T * C * 4 > 150 KB
  each with the flag patterns none / leading / trailing, both / every gap / a star between equal labels, consecutive stars /
  a star-only row / an empty row, at penalty 0 and -0.5.

Then: status 2 (a bad entry) and status 1 (no path) with and without zero_infinity; star-free rows against w2l_ctc_loss's own
output; and the model level -- a Wav2Letter with model.wildcard='*' whose training_step's loss is WildcardCTCLoss on the forward
output, and whose replayed steps end on the parameters of the same steps run eagerly, bit for bit."""
import numpy as np
import pytest
import torch

import wctc_refs as R
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
        pytest.exit(f'HIP error in a direct wctc launch, nothing more is run: {e}', returncode=3)


def bounded(case, got, ref, bound):
    ok, g, r = split_nonfinite(got, ref)
    assert ok, f'{case}: inf / NaN pattern differs from the reference'
    return record('wctc', case, ratio(g, r, np.where(np.isfinite(bound), bound, 0.0)))


def wctc_run(L, c, want_grad=True):
    N, T, C = c.dims
    lp, tg = up(c.lp), up(c.targets, torch.int32)
    il, tl = up(c.in_len, torch.int32), up(c.tg_len, torch.int32)
    nll, loss, status = Buf((N,)), Buf((1,)), Buf((N,), torch.int32)
    grad = Buf((N, T, C)) if want_grad else None
    nbytes = L.lib.w2l_wctc_workspace_bytes(N, T, c.Smax)
    assert nbytes == 2 * N * T * (2 * c.Smax + 1) * 4 + N * (2 * c.Smax + 2) * 4
    ws = Buf((nbytes // 4,))
    run(L, L.lib.w2l_wctc_loss(p(L, lp), p(L, tg), p(L, il), p(L, tl), N, T, C, c.Smax, R.BLANK, c.zero_inf, R.STAR, c.penalty,
                               p(L, nll), p(L, loss), p(L, grad), p(L, status), p(L, ws), L.stream_ptr()))
    assert guards(lp, tg, il, tl, nll, loss, status, grad, ws), f'{c.name}: a guard region was written'
    return nll.np(), float(loss.np()[0]), status.np(), None if grad is None else grad.np()


def wctc_check(L, c):
    r = R.case_ref(c)
    nll, loss, status, grad = wctc_run(L, c)
    assert status.tolist() == r['status'].tolist(), c.name
    rs = [bounded(c.name + '-nll', nll, r['nll'], r['nll_b']),
          bounded(c.name + '-loss', np.array([loss]), np.array([r['loss']]), np.array([r['loss_b']]))]
    for n in range(c.dims[0]):
        assert not grad[n, r['Tn'][n]:].any(), 'gradient rows past the input length must be exactly 0'
    spec = ~np.isnan(r['grad'])                         # an infinite utterance without zero_infinity: its gradient is not specified
    rs.append(bounded(c.name + '-grad', grad[spec], r['grad'][spec], r['grad_b'][spec]))
    return max(rs), (nll, loss, status, grad)


@pytest.mark.parametrize('shape,group,penalty', R.shape_cases(),
                         ids=lambda v: v if isinstance(v, str) else f'{v:g}')
def test_wctc_shapes_and_patterns(L, shape, group, penalty):
    c = R.shape_case(shape, group, penalty)
    print(c.name, 'variant (NT, SPT, LP_LDS):', c.variant)
    worst, (nll, _, _, grad) = wctc_check(L, c)
    assert worst <= 1.0
    # the gradient sums to zero over the classes (w2l_log_softmax_bwd then passes it through): the reference's rows sum to zero,
    # so a device row's sum is at most the sum of its elements' bounds
    assert (np.abs(grad.astype(np.float64).sum(axis=2)) <= R.case_ref(c)['grad_b'].sum(axis=2) + 1e-12).all()


def test_bad_entry_is_status_2_and_contributes_nothing(L):
    c = R.bad_entry_case()
    worst, (nll, loss, status, grad) = wctc_check(L, c)
    assert worst <= 1.0
    assert status.tolist() == [0, 2, 2, 2, 0]
    assert not nll[1:4].any() and not grad[1:4].any() and grad[0].any() and grad[4].any()


@pytest.mark.parametrize('zero_inf', [1, 0])
def test_infeasible_row_is_status_1_and_obeys_zero_infinity(L, zero_inf):
    c = R.infeasible_case(zero_inf)
    worst, (nll, loss, status, grad) = wctc_check(L, c)
    assert worst <= 1.0
    assert status.tolist() == [1, 1, 0, 1]
    if zero_inf:
        assert not nll[[0, 1, 3]].any() and np.isfinite(loss) and not grad[[0, 1, 3]].any() and grad[2].any()
    else:
        assert np.isinf(nll[[0, 1, 3]]).all() and np.isinf(loss) and np.isfinite(nll[2]) and np.isfinite(grad[2]).all()


def test_rejected_arguments_write_nothing(L):
    c = R.shape_case(0, 0, 0.0)
    N, T, C = c.dims
    lp, tg, il, tl = up(c.lp), up(c.targets, torch.int32), up(c.in_len, torch.int32), up(c.tg_len, torch.int32)
    nll, loss, status, grad = Buf((N,)), Buf((1,)), Buf((N,), torch.int32), Buf((N, T, C))
    ws = Buf((L.lib.w2l_wctc_workspace_bytes(N, T, c.Smax) // 4,))
    for star, penalty, word in ((R.BLANK, 0.0, 'blank'), (R.STAR, 0.5, 'penalty')):
        rc = L.lib.w2l_wctc_loss(p(L, lp), p(L, tg), p(L, il), p(L, tl), N, T, C, c.Smax, R.BLANK, 1, star, penalty, p(L, nll),
                                 p(L, loss), p(L, grad), p(L, status), p(L, ws), L.stream_ptr())
        torch.cuda.synchronize()
        assert rc != 0 and word in last_error(L)
    assert torch.isnan(grad.flat).all() and torch.isnan(loss.flat).all()
    assert L.lib.w2l_wctc_workspace_bytes(N, T, 4096) > 0 and L.lib.w2l_wctc_loss(
        p(L, lp), p(L, tg), p(L, il), p(L, tl), N, T, C, 4096, R.BLANK, 1, R.STAR, 0.0, p(L, nll), p(L, loss), p(L, grad),
        p(L, status), p(L, ws), L.stream_ptr()) != 0 and '4095' in last_error(L)


@pytest.mark.parametrize('shape', range(len(R.SHAPES)), ids=[s[0] for s in R.SHAPES])
def test_star_free_rows_agree_with_ctc_loss(L, shape):
    """the same rows through w2l_ctc_loss: both lie within their bounds of the same reference, so they differ by at most the sum
    of the two (frontend_refs.ctc_ref's and wctc_ref's).  Whether they are bit-equal is printed, not asserted."""
    import frontend_refs as FR
    c = R.star_free_case(shape)
    worst, (nll, loss, status, grad) = wctc_check(L, c)
    assert worst <= 1.0 and not status.any()
    N, T, C = c.dims
    lp, tg = up(c.lp), up(c.targets, torch.int32)
    il, tl = up(c.in_len, torch.int32), up(c.tg_len, torch.int32)
    nll2, loss2, grad2 = Buf((N,)), Buf((1,)), Buf((N, T, C))
    ws = Buf((L.lib.w2l_ctc_workspace_bytes(N, T, c.Smax) // 4,))
    run(L, L.lib.w2l_ctc_loss(p(L, lp), p(L, tg), p(L, il), p(L, tl), N, T, C, c.Smax, R.BLANK, c.zero_inf, p(L, nll2), p(L, loss2),
                              p(L, grad2), p(L, ws), L.stream_ptr()))
    assert guards(lp, tg, il, tl, nll2, loss2, grad2, ws)
    w, k = R.case_ref(c), FR.ctc_ref(c.lp, c.targets, c.in_len, c.tg_len, R.BLANK, c.zero_inf, c.Smax)
    assert np.array_equal(w['nll'], k['nll']) and np.array_equal(w['grad'], k['grad'])          # one reference, two bounds
    assert ratio(nll, nll2.np().astype(np.float64), w['nll_b'] + k['nll_b']) <= 1.0
    assert ratio(grad, grad2.np().astype(np.float64), w['grad_b'] + k['grad_b']) <= 1.0
    assert abs(loss - float(loss2.np()[0])) <= w['loss_b'] + k['loss_b']
    equal = np.array_equal(nll, nll2.np()) and np.array_equal(grad, grad2.np()) and loss == float(loss2.np()[0])
    print(f'BITEQUAL {c.name}: w2l_wctc_loss {"==" if equal else "!="} w2l_ctc_loss '
          f'(max |d nll| {np.abs(nll - nll2.np()).max():.3g}, max |d grad| {np.abs(grad - grad2.np()).max():.3g})')


# ---- model level ----------------------------------------------------------------------------------------------------------------------

def _bit_reproducible(monkeypatch):
    from wav2letter_pytorch_amd import engine as E
    monkeypatch.setattr(E, 'FOLD_BN_FWD', '0')
    monkeypatch.setattr(E, 'FAST_BN_BWD', False)
    monkeypatch.setattr(E, 'DETERMINISTIC_WGRAD', True)


def _wild_model_and_batches():
    from oracle import w2l_oracle as O
    from wav2letter_pytorch_amd import Wav2Letter
    from wav2letter_pytorch_amd.config import to_cfg
    labels = O.ENGLISH_LOWERCASE
    layers = [(128, 11, 2, 1, 0.0)]                                          # mid_layers = 1
    sd = O.init_wav2letter_state(layers, seed=71)
    cfg = to_cfg(dict(name='wav2letter', mid_layers=1, input_size=64, labels=labels, precision='bf16', wildcard='*',
                      wildcard_penalty=-0.25,
                      layers=[dict(output_size=c, kernel_size=k, stride=s, dilation=d, dropout=0.0) for c, k, s, d, _ in layers],
                      audio_conf=dict(window='hamming', window_stride=0.01, window_size=0.02, sample_rate=16000),
                      decoder=dict(_target_='decoder.GreedyDecoder', labels=labels),
                      optimizer=dict(_target_='torch.optim.SGD', lr=1e-5, momentum=0.9, nesterov=True, weight_decay=1e-5),
                      scheduler=dict(_target_='torch.optim.lr_scheduler.ExponentialLR', gamma=0.999)))

    def make():
        model = Wav2Letter(cfg)
        model.load_state_dict({k: v.clone() for k, v in sd.items()})
        return model.cuda()

    star = len(labels)
    batches = []
    for b in range(2):
        x, il, tg, tl = O.synthetic_batch(4, 240, seed=72 + b, s_lo=8, s_hi=20)
        rows = [tg[n, :int(tl[n])].tolist() for n in range(4)]
        rows[0] = [star] + rows[0] + [star]                                  # both ends
        rows[1] = rows[1][:3] + [star, star] + rows[1][3:]                   # consecutive stars inside
        rows[2] = rows[2] + [star]                                           # trailing; row 3 has none
        tl = torch.tensor([len(r) for r in rows], dtype=torch.int32)
        tg = torch.zeros(4, int(tl.max()), dtype=torch.int32)
        for n, r in enumerate(rows):
            tg[n, :len(r)] = torch.tensor(r, dtype=torch.int32)
        texts = tuple(''.join('*' if i == star else labels[i] for i in r) for r in rows)
        batches.append((x, il, tg, tl, tuple('f%d' % k for k in range(4)), texts))
    return make, batches, star


def test_model_step_loss_is_the_wildcard_criterion(monkeypatch):
    from wav2letter_pytorch_amd.ctc_loss import WildcardCTCLoss
    from wav2letter_pytorch_amd.optim import FusedSGD
    _bit_reproducible(monkeypatch)
    make, batches, star = _wild_model_and_batches()
    torch.manual_seed(3)
    model = make().train()
    model.check_nan = False
    model.async_metrics = False
    assert type(model.criterion) is WildcardCTCLoss and model.criterion.penalty == -0.25
    model._optimizers = FusedSGD.from_sgd(torch.optim.SGD(model.parameters(), lr=0.02, momentum=0.9, nesterov=True))
    x, il, tg, tl, _, texts = batches[0]
    out, ol = model(x.cuda(), il)
    out, ol = out.detach(), torch.as_tensor(ol).cpu()
    want = WildcardCTCLoss(blank=0, reduction='mean', zero_infinity=True, penalty=-0.25)(out.transpose(0, 1), tg, ol, tl)
    loss = model.training_step(batches[0], 0)
    assert float(loss.detach()) == float(want)                                        # the same forward, the same criterion: bit for bit
    assert model.criterion.last_status().tolist() == [0, 0, 0, 0]
    # ... which is the reference's value of the forward output, and its gradient reaches the logits
    r = R.wctc_ref(out.float().cpu().numpy(), tg.numpy(), ol.numpy(), tl.numpy(), 0, 1, tg.shape[1], star, -0.25)
    assert abs(float(loss) - r['loss']) <= r['loss_b']
    loss.backward()
    # the string metrics were scored against the transcripts without the mark
    logged = dict(model._logged)
    assert np.isfinite([logged['train_cer'], logged['train_wer'], logged['train_len_ratio']]).all()
    hyp_len = logged['train_len_ratio'] * sum(len(t) for t in model.metric_texts(texts))
    assert abs(hyp_len - round(hyp_len)) < 1e-6 and all('*' not in t for t in model.metric_texts(texts))


def _train(make, batches, steps, replay_on):
    from wav2letter_pytorch_amd import _lib, replay
    from wav2letter_pytorch_amd.optim import FusedSGD
    replay.ENABLED = replay_on
    _lib.AUDIT = replay_on
    for k in ('recorded', 'replayed_F', 'replayed_B', 'replayed_O', 'replayed_X'):
        replay.STATS[k] = 0
    replay.STATS['poisoned'] = []
    try:
        torch.manual_seed(11)
        model = make().train()
        model.check_nan = False
        opt = FusedSGD.from_sgd(torch.optim.SGD(model.parameters(), lr=0.02, momentum=0.9, nesterov=True, weight_decay=1e-4))
        model._optimizers = opt
        losses = []
        for i in range(steps):
            batch = batches[i % len(batches)]
            opt.zero_grad(set_to_none=True)
            loss = model.training_step(batch, i)
            loss.backward()
            opt.step()
            model.on_train_batch_end(loss, batch, i)
            losses.append(float(loss))
        opt.join()
        model.resolve_metrics(wait_all=True)
        torch.cuda.synchronize()
        if replay_on:
            bad = replay.audit(model.engine())
            assert bad == [], bad[:8]
        return losses, {k: v.detach().cpu().numpy().copy() for k, v in model.state_dict().items()}, dict(replay.STATS)
    finally:
        replay.ENABLED = True
        _lib.AUDIT = False


def test_replayed_wildcard_steps_equal_eager_steps(monkeypatch):
    """the loss call sits between the replayed forward and backward phases, outside any recording: eight steps over two star
    batches, replayed and eager, give the same losses and end on the same parameters, bit for bit"""
    _bit_reproducible(monkeypatch)
    make, batches, _ = _wild_model_and_batches()
    le, pe, _ = _train(make, batches, 8, False)
    lr_, pr, st = _train(make, batches, 8, True)
    assert st['poisoned'] == [], st
    assert st['recorded'] >= 1 and st['replayed_F'] >= 2 and st['replayed_B'] >= 2, st
    assert np.isfinite(le).all() and le == lr_, (le, lr_)
    for k in pe:
        assert np.array_equal(pe[k], pr[k]), k
