"""Fused Adam / AdamW without a GPU: the float64 reference the device tests lean on (tests/adam_refs.py) pinned to
torch.optim.Adam / AdamW in float64, its bound shown to catch planted defects, the host model of w2l_adam_tick against the
closed form, the replay table, optim.FusedAdamW's state dict through a plain torch.optim.AdamW, the Trainer's scheduler plan
and what configure_optimizers returns under model.scheduler_interval."""
import copy
import math
import os
import sys

import numpy as np
import pytest
import torch

import adam_refs as A
import kernel_refs as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LR = 1e-3


def rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(np.asarray(b)).max(), 1e-300))


def _closed_dyn(t, lr, b1, b2):
    return [lr, lr / (1.0 - b1 ** t), math.sqrt(1.0 - b2 ** t)]


def _inputs(n=257, seed=5):
    g = torch.Generator().manual_seed(seed)
    p, gr, m = (torch.randn(n, generator=g) for _ in range(3))
    v = torch.randn(n, generator=g) ** 2
    gr[::97] = 0.0
    v[::89] = 0.0
    return p.double().numpy(), gr.double().numpy(), m.double().numpy(), v.double().numpy()


@pytest.mark.parametrize('clip', [None, (0.5, 0.25)])
@pytest.mark.parametrize('step', [1, 2, 1000])
@pytest.mark.parametrize('wd', [0.0, 1e-2])
@pytest.mark.parametrize('decoupled', [0, 1])
def test_adam_ref_matches_torch_float64(decoupled, wd, step, clip):
    """one step of torch.optim.Adam / AdamW on float64 tensors whose state says ``step - 1`` steps have been taken, the clip
    written as torch's clip_grad_norm_ / clip_grad_value_ do it; step 1 starts from torch's own fresh state (zero moments)"""
    p0, g0, m0, v0 = _inputs()
    if step == 1:
        m0, v0 = np.zeros_like(m0), np.zeros_like(v0)
    b1, b2, eps, wdf = R.f32(A.ADAM_BETAS[0]), R.f32(A.ADAM_BETAS[1]), R.f32(A.ADAM_EPS), R.f32(wd)
    p = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    cls = torch.optim.AdamW if decoupled else torch.optim.Adam
    opt = cls([p], lr=LR, betas=(b1, b2), eps=eps, weight_decay=wdf)
    if step > 1:
        p.grad = torch.zeros_like(p)
        opt.step()                                    # creates the state; overwritten below
        with torch.no_grad():
            p.copy_(torch.from_numpy(p0))
        st = opt.state[p]
        st['step'].fill_(step - 1)
        st['exp_avg'].copy_(torch.from_numpy(m0))
        st['exp_avg_sq'].copy_(torch.from_numpy(v0))
    p.grad = torch.from_numpy(g0.copy())
    if clip is not None:
        p.grad.mul_(R.f32(clip[0])).clamp_(-R.f32(clip[1]), R.f32(clip[1]))
    opt.step()
    P, M, V = A.adam_ref(p0, g0, m0, v0, _closed_dyn(step, LR, b1, b2), b1, b2, eps, wd, decoupled, *(clip or (None, None)))
    assert rel(M.v, opt.state[p]['exp_avg'].numpy()) <= 1e-12
    assert rel(V.v, opt.state[p]['exp_avg_sq'].numpy()) <= 1e-12
    assert rel(P.v, p.detach().numpy()) <= 1e-12
    assert (M.a >= np.abs(M.v)).all() and (V.a >= np.abs(V.v)).all() and np.isfinite(P.v).all()
    assert (P.bound() >= 0).all() and np.isfinite(P.bound()).all()


def _fp32_dyn(t, lr, b1, b2):
    return [float(np.float32(x)) for x in A.tick_host(t, lr, b1, b2)[3]]


@pytest.mark.parametrize('decoupled,wd,step', [(0, 1e-2, 1), (1, 1e-2, 1), (0, 0.0, 1000), (1, 1e-2, 1000)])
def test_adam_bound_admits_fp32_and_catches_defects(decoupled, wd, step):
    """the rule evaluated in NumPy float32, operation by operation as the kernel writes it, lies within the bound; the same
    with a planted defect -- the second bias correction left out, the weight decay applied after the moments, beta2 used for
    the first moment -- does not"""
    p0, g0, m0, v0 = _inputs(4096, seed=9)
    b1, b2 = A.ADAM_BETAS
    dyn = _fp32_dyn(step, LR, b1, b2)
    P, M, V = A.adam_ref(p0, g0, m0, v0, dyn, b1, b2, A.ADAM_EPS, wd, decoupled)
    f = np.float32

    def device(defect=None):
        p, g, m, v = (x.astype(f) for x in (p0, g0, m0, v0))
        lr, s1, s2 = (f(x) for x in dyn)
        fb1, fb2, eps, fwd = f(b1), f(b2), f(A.ADAM_EPS), f(wd)
        if defect == 'no_bc2':
            s2 = f(1.0)
        if decoupled:
            p = p * (f(1) - lr * fwd)
        elif defect != 'wd_late':
            g = g + fwd * p
        m = (fb2 if defect == 'beta' else fb1) * m + (f(1) - fb1) * g
        v = fb2 * v + (f(1) - fb2) * (g * g)
        if defect == 'wd_late' and not decoupled:
            g = g + fwd * p
            m = m + (f(1) - fb1) * fwd * p
        return p - s1 * (m / (np.sqrt(v) / s2 + eps)), m, v

    def worst(out):
        return max(float((np.abs(o.astype(np.float64) - r.v) / np.maximum(r.bound(), 1e-300)).max()) for o, r in zip(out, (P, M, V)))

    assert worst(device()) <= 1.0
    assert worst(device('no_bc2')) > 10.0
    assert worst(device('beta')) > 10.0
    if not decoupled and wd:
        assert worst(device('wd_late')) > 10.0


@pytest.mark.parametrize('betas', [(0.9, 0.999), (0.95, 0.5)])
def test_tick_host_model_against_closed_form(betas):
    """the running products and the dyn scalars formed from them agree with 1 - beta**t to 1e-12 relative"""
    b1, b2 = betas
    for t in (1, 2, 3, 1000):
        step, pow1, pow2, dyn = A.tick_host(t, 3e-4, b1, b2)
        assert step == t
        for got, want in ((1.0 - pow1, 1.0 - b1 ** t), (1.0 - pow2, 1.0 - b2 ** t),
                          (dyn[1], 3e-4 / (1.0 - b1 ** t)), (dyn[2], math.sqrt(1.0 - b2 ** t))):
            assert abs(got - want) <= 1e-12 * abs(want), (t, got, want)
        assert dyn[0] == 3e-4


def test_replay_table_has_the_updates_not_the_tick():
    from wav2letter_pytorch_amd import _lib
    assert _lib.lib.w2l_replay_op(b'w2l_adam_pack') >= 0
    assert _lib.lib.w2l_replay_op(b'w2l_adam_small_multi') >= 0
    assert _lib.lib.w2l_replay_op(b'w2l_adam_tick') == -1
    assert _lib.lib.w2l_abi_version() == 2
    ops = _lib._replay_ops()
    assert len(ops['w2l_adam_pack'][1]) == 23 <= _lib.REPLAY_MAX_ARGS and len(ops['w2l_adam_small_multi'][1]) == 11


def _step_both(ours, theirs, ps, qs, gen, skip=None):
    for i, (x, y) in enumerate(zip(ps, qs)):
        g = torch.randn(x.shape, generator=gen)
        x.grad, y.grad = (None, None) if i == skip else (g.clone(), g.clone())
    ours.step()
    theirs.step()


@pytest.mark.parametrize('cls', [torch.optim.Adam, torch.optim.AdamW])
def test_state_dict_round_trips_through_torch(cls):
    """host tensors take torch's own rule inside FusedAdamW: same trajectory as torch (a parameter that misses a gradient
    keeps its own step count), a state dict torch.optim loads as it is, and one FusedAdamW loads back from torch"""
    from wav2letter_pytorch_amd.optim import FusedAdamW
    gen = torch.Generator().manual_seed(2)
    ps = [torch.nn.Parameter(torch.randn(5, 3, generator=gen)), torch.nn.Parameter(torch.randn(7, generator=gen))]
    qs = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    kw = dict(lr=1e-2, weight_decay=1e-2, betas=(0.9, 0.99))
    ours, theirs = FusedAdamW.from_adam(cls(ps, **kw)), cls(qs, **kw)
    assert ours.param_groups[0]['decoupled_weight_decay'] == (cls is torch.optim.AdamW)
    for i in range(4):
        _step_both(ours, theirs, ps, qs, gen, skip=1 if i == 2 else None)
    for x, y in zip(ps, qs):
        assert torch.allclose(x, y, rtol=1e-6, atol=1e-7)
    assert [ours.state[p]['step'] for p in ps] == [4, 3]
    sd = ours.state_dict()
    assert set(sd) == {'state', 'param_groups'} and set(sd['state'][0]) == {'step', 'exp_avg', 'exp_avg_sq'}
    assert all(torch.is_tensor(s['step']) and s['step'].device.type == 'cpu' for s in sd['state'].values())
    assert isinstance(ours.state[ps[0]]['step'], int)                  # the live state keeps its host count
    fresh = cls(qs, **kw)
    fresh.load_state_dict(sd)
    assert [float(fresh.state[q]['step']) for q in qs] == [4.0, 3.0]
    for p, q in zip(ps, qs):
        assert torch.equal(fresh.state[q]['exp_avg'], ours.state[p]['exp_avg'])
    back = FusedAdamW.from_adam(cls(ps, **kw))
    back.load_state_dict(copy.deepcopy(theirs.state_dict()))     # (as a checkpoint file would: no tensor shared)
    assert [back.state[p]['step'] for p in ps] == [4, 3]
    gs = back._scalars(0)
    assert gs['count'] == 4 and gs['pow1'] == A.tick_host(4, 0, 0.9, 0.99)[1] and gs['pow2'] == A.tick_host(4, 0, 0.9, 0.99)[2]
    _step_both(back, theirs, ps, qs, gen)
    for x, y in zip(ps, qs):
        assert torch.allclose(x, y, rtol=1e-6, atol=1e-7)


def test_from_adam_refuses_what_the_kernels_do_not_do():
    from wav2letter_pytorch_amd.optim import FusedAdamW
    p = [torch.nn.Parameter(torch.zeros(3))]
    with pytest.raises(ValueError):
        FusedAdamW.from_adam(torch.optim.Adam(p, amsgrad=True))
    with pytest.raises(ValueError):
        FusedAdamW.from_adam(torch.optim.AdamW(p, maximize=True))
    with pytest.raises(TypeError):
        FusedAdamW.from_adam(torch.optim.SGD(p, lr=0.1))


def test_step_under_graph_capture_is_refused(monkeypatch):
    """a captured step would replay the captured step's bias corrections for good: step() raises before it counts or launches
    anything (as torch.optim.Adam with capturable=False does)"""
    from wav2letter_pytorch_amd.optim import FusedAdamW
    p = torch.nn.Parameter(torch.ones(3))
    opt = FusedAdamW.from_adam(torch.optim.AdamW([p], lr=1e-3))
    p.grad = torch.ones(3)
    opt.step()
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: True)
    monkeypatch.setattr(torch.cuda, 'is_current_stream_capturing', lambda: True)
    before = p.detach().clone()
    with pytest.raises(RuntimeError, match='capture'):
        opt.step()
    assert torch.equal(p.detach(), before) and opt.state[p]['step'] == 1 and opt._scalars(0)['count'] == 1


def test_replay_signature_leaves_the_learning_rate_out():
    from wav2letter_pytorch_amd import replay
    from wav2letter_pytorch_amd.optim import FusedAdamW, FusedSGD
    p = [torch.nn.Parameter(torch.zeros(3))]
    adam = FusedAdamW.from_adam(torch.optim.AdamW(p, lr=1e-3))
    a = replay.opt_signature(adam)
    adam.param_groups[0]['lr'] = 5e-4
    assert replay.opt_signature(adam) == a and a[-1] is None
    adam.param_groups[0]['eps'] = 1e-6
    assert replay.opt_signature(adam) != a
    sgd = FusedSGD.from_sgd(torch.optim.SGD(p, lr=0.1, momentum=0.9))
    s = replay.opt_signature(sgd)
    assert s == ((0.1, 0.9, 0, False, 0, False), 0, None)
    sgd.param_groups[0]['lr'] = 0.05
    assert replay.opt_signature(sgd) != s
    assert 'recorded_O' in replay.STATS


def test_trainer_scheduler_plan():
    from wav2letter_pytorch_amd.trainer import scheduler_plan
    s1, s2 = object(), object()
    assert scheduler_plan([s1]) == [(s1, 'epoch', 1)]
    assert scheduler_plan([s1, {'scheduler': s2, 'interval': 'step', 'frequency': 3}]) == [(s1, 'epoch', 1), (s2, 'step', 3)]
    assert scheduler_plan([{'scheduler': s2}]) == [(s2, 'epoch', 1)]
    assert scheduler_plan(None) == [] and scheduler_plan([]) == []
    for bad in ({'scheduler': s1, 'interval': 'batch'}, {'scheduler': s1, 'interval': 'step', 'frequency': 0}, {'interval': 'step'}):
        with pytest.raises(ValueError):
            scheduler_plan([bad])


def _model_cfg(**kw):
    from wav2letter_pytorch_amd.config import to_cfg
    from wav2letter_pytorch_amd.data import label_sets
    labels = label_sets.labels_map['english_lowercase']
    d = dict(name='wav2letter', mid_layers=1, input_size=64, labels=labels,
             layers=[dict(output_size=64, kernel_size=11, stride=2, dilation=1, dropout=0.0)] * 3,
             audio_conf=dict(window='hamming', window_stride=0.01, window_size=0.02, sample_rate=16000),
             decoder=dict(_target_='decoder.GreedyDecoder', labels=labels),
             optimizer=dict(_target_='torch.optim.AdamW', lr=1e-3, weight_decay=1e-2),
             scheduler=dict(_target_='torch.optim.lr_scheduler.ExponentialLR', gamma=0.999))
    d.update(kw)
    return to_cfg(d)


def test_configure_optimizers_scheduler_interval():
    from wav2letter_pytorch_amd import Wav2Letter
    from wav2letter_pytorch_amd.train import build_config
    opts, schs = Wav2Letter(_model_cfg()).configure_optimizers()
    assert type(opts[0]) is torch.optim.AdamW                       # (host parameters: torch's optimizer as it is)
    assert isinstance(schs[0], torch.optim.lr_scheduler.ExponentialLR)
    opts, schs = Wav2Letter(_model_cfg(scheduler_interval='epoch')).configure_optimizers()
    assert isinstance(schs[0], torch.optim.lr_scheduler.ExponentialLR)
    opts, schs = Wav2Letter(_model_cfg(scheduler_interval='step')).configure_optimizers()
    assert set(schs[0]) == {'scheduler', 'interval', 'frequency'} and schs[0]['interval'] == 'step' and schs[0]['frequency'] == 1
    assert isinstance(schs[0]['scheduler'], torch.optim.lr_scheduler.ExponentialLR)
    with pytest.raises(ValueError):
        Wav2Letter(_model_cfg(scheduler_interval='batch')).configure_optimizers()
    assert build_config(['model.scheduler_interval=step']).model.scheduler_interval == 'step'
    with pytest.raises(ValueError):
        build_config(['model.scheduler_interval=batch'])
