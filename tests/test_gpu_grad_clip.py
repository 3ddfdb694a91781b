"""Gradient clipping (torch.nn.utils.clip_grad_norm_ / clip_grad_value_, Lightning's Trainer(gradient_clip_val=)) on a real
MI355X: the one-launch device norm (w2l_grad_sqnorm_multi) against float64 NumPy and torch, optim.FusedSGD's clipped step
against torch.optim.SGD after torch's clipping, with held-back weight gradients, under recorded launch lists, for Novograd (the
generic path), through trainer.Trainer, Lightning's hook and the data-parallel reducer."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from gpu_helpers import build_w2l, scale_err

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
LAYERS = [(128, 11, 2, 1, 0.0), (128, 13, 1, 2, 0.0), (192, 5, 1, 1, 0.0)]
KW = dict(lr=0.05, momentum=0.9, nesterov=True, weight_decay=1e-3)


@pytest.fixture(autouse=True)
def _restore_library_wgrad_mode():
    """the step engine hands its weight-gradient mode to the library at every backward pass (w2l_wgrad_deterministic), and
    the library keeps it: a test that runs the bit-reproducible step must not leave deterministic mode on for the tests that
    follow (monkeypatch restores the Python flag only)"""
    from wav2letter_pytorch_amd import engine as E
    from wav2letter_pytorch_amd._lib import lib
    mode = int(E.DETERMINISTIC_WGRAD)
    yield
    lib.w2l_wgrad_deterministic(mode)


def _bit_reproducible(monkeypatch):
    from wav2letter_pytorch_amd import engine as E
    monkeypatch.setattr(E, 'FOLD_BN_FWD', '0')
    monkeypatch.setattr(E, 'FAST_BN_BWD', False)
    monkeypatch.setattr(E, 'DETERMINISTIC_WGRAD', True)


def _device_norm(grads, inf_norm=False, max_norm=1.0):
    """w2l_grad_sqnorm_multi over ``grads`` -> the clip buffer [norm, coef, bound, -] on the host"""
    from wav2letter_pytorch_amd import _lib
    from wav2letter_pytorch_amd._lib import check, lib, ptr, stream_ptr
    flat, c0 = [], 0
    for g in grads:
        flat += [g.data_ptr(), g.numel(), c0]
        c0 += -(-g.numel() // _lib.GNORM_CHUNK)
    table = torch.tensor(flat, dtype=torch.int64).cuda()
    partials = torch.empty(_lib.GNORM_BLOCKS, dtype=torch.float64, device='cuda')
    buf = torch.zeros(4, dtype=torch.float32, device='cuda')
    out = torch.empty((), dtype=torch.float32, device='cuda')
    check(lib.w2l_grad_sqnorm_multi(ptr(table), len(grads), c0, int(inf_norm), ptr(partials), float(max_norm), ptr(buf), ptr(out),
                                    stream_ptr()), 'w2l_grad_sqnorm_multi')
    torch.cuda.synchronize()
    b = buf.cpu().numpy()
    assert np.array_equal(b[0], out.cpu().numpy(), equal_nan=True)
    return b


def _awkward_grads():
    gen = torch.Generator().manual_seed(5)
    sizes = [1, 63, 64, 65, 4095, 8192, 8193, 1000, 3, 77777, 129, 2048, 12345, 511, 7, 300000]
    gs = [torch.randn(n, generator=gen).cuda() for n in sizes]
    tap = torch.empty(11, 64, 64, device='cuda').normal_(generator=None).permute(1, 2, 0)     # [Cout, Cin, Kw] tap-major
    gs.append(tap)
    gs.append(torch.randn(10 ** 6 + 3, generator=gen).cuda() * 1e-2)
    big = torch.randn(20001, generator=gen).cuda()
    gs.append(big[1:])                                                         # 4-byte aligned only: no float4 path
    gs.append(torch.randn(3, 5, generator=gen).cuda())
    return gs


def _torch_norm(gs, max_norm, norm_type=2.0):
    """torch.nn.utils.clip_grad_norm_ over parameters whose gradients are copies of ``gs``: its returned total norm"""
    ps = []
    for g in gs:
        p = torch.zeros_like(g, requires_grad=True)
        p.grad = g.clone()
        ps.append(p)
    return torch.nn.utils.clip_grad_norm_(ps, max_norm, norm_type=norm_type)


def test_norm_kernel_matches_float64_and_torch():
    gs = _awkward_grads()
    ref = np.concatenate([g.detach().cpu().numpy().astype(np.float64).ravel() for g in gs])
    b = _device_norm(gs, max_norm=0.5)
    n2 = math.sqrt(float((ref * ref).sum()))
    assert abs(float(b[0]) - n2) <= 1e-6 * n2, (b[0], n2)
    assert b[1] == np.float32(0.5) / (np.float32(b[0]) + np.float32(1e-6)) and b[2] == np.inf
    again = _device_norm(gs, max_norm=0.5)
    assert again.tobytes() == b.tobytes()                                      # deterministic, bit for bit
    bi = _device_norm(gs, inf_norm=True, max_norm=0.5)
    assert bi[0] == np.float32(np.abs(ref).max())
    torch_norm = _torch_norm(gs, 0.5)
    assert abs(float(torch_norm) - float(b[0])) <= 1e-5 * n2
    for bad in (float('inf'), float('nan')):
        gb = [g.clone() for g in gs]
        gb[9][123] = bad
        for inf_norm in (False, True):
            bb = _device_norm(gb, inf_norm=inf_norm, max_norm=0.5)
            tn = _torch_norm(gb, 0.5, norm_type=float('inf') if inf_norm else 2.0)
            tc = torch.clamp(0.5 / (tn + 1e-6), max=1.0)
            assert np.array_equal(bb[0], tn.cpu().numpy(), equal_nan=True), (bad, inf_norm, bb, tn)
            assert np.array_equal(bb[1], tc.cpu().numpy(), equal_nan=True), (bad, inf_norm, bb, tc)
        assert (bb[1] == 0) if bad == float('inf') else np.isnan(bb[1])


def _clip_call(opt, mode, val):
    if isinstance(opt, torch.optim.SGD) and hasattr(opt, 'clip_grad_norm_'):
        return opt.clip_grad_norm_(val) if mode == 'norm' else opt.clip_grad_value_(val)
    params = [p for g in opt.param_groups for p in g['params'] if p.grad is not None]
    if mode == 'norm':
        return torch.nn.utils.clip_grad_norm_(params, val)
    torch.nn.utils.clip_grad_value_(params, val)
    return None


@pytest.mark.parametrize('mode', ['norm', 'value'])
@pytest.mark.parametrize('overlap', [True, False])
def test_fused_clipped_step_matches_torch(mode, overlap):
    from oracle import w2l_oracle as O
    from wav2letter_pytorch_amd.optim import FusedSGD
    sd = O.init_wav2letter_state(LAYERS, seed=4)
    ma = build_w2l(LAYERS, sd, 'bf16').train()
    mb = build_w2l(LAYERS, sd, 'bf16').train()
    oa = FusedSGD.from_sgd(torch.optim.SGD(ma.parameters(), **KW))
    oa.overlap = overlap
    ob = torch.optim.SGD(mb.parameters(), **KW)
    val = 1e-3
    x, il, tg, tl = O.synthetic_batch(2, 160, seed=11, s_lo=5, s_hi=15)
    for it in range(3):
        norms = []
        for m, o in ((ma, oa), (mb, ob)):
            o.zero_grad(set_to_none=True)
            out, ol = m(x.cuda(), il)
            m.criterion(out.transpose(0, 1), tg, ol, tl).backward()
            norms.append(_clip_call(o, mode, val))
            o.step()
        if mode == 'norm':
            na, nb = float(norms[0]), float(norms[1])
            assert abs(na - nb) <= 1e-5 * nb and nb > 4 * val, (it, na, nb)       # the coefficient is well below 1
        else:
            assert norms == [None, None]
    oa.join()
    for (k, pa), (_, pb) in zip(ma.named_parameters(), mb.named_parameters()):
        assert scale_err(pa.detach().cpu().numpy(), pb.detach().cpu().numpy()) < 2e-5, k
        ba, bb = oa.state[pa]['momentum_buffer'], ob.state[pb]['momentum_buffer']
        assert scale_err(ba.detach().cpu().numpy(), bb.detach().cpu().numpy()) < 2e-5, k


def test_noop_clip_is_bit_identical(monkeypatch):
    """max_norm = 1e30: coefficient 1, bound +inf -- the clipped update kernels must then change nothing, bit for bit"""
    from oracle import w2l_oracle as O
    from wav2letter_pytorch_amd.optim import FusedSGD
    _bit_reproducible(monkeypatch)
    sd = O.init_wav2letter_state(LAYERS, seed=6)
    res = []
    for armed in (False, True):
        m = build_w2l(LAYERS, sd, 'bf16').train()
        o = FusedSGD.from_sgd(torch.optim.SGD(m.parameters(), **KW))
        o.overlap = True
        x, il, tg, tl = O.synthetic_batch(2, 160, seed=12, s_lo=5, s_hi=15)
        for _ in range(3):
            o.zero_grad(set_to_none=True)
            out, ol = m(x.cuda(), il)
            m.criterion(out.transpose(0, 1), tg, ol, tl).backward()
            if armed:
                o.clip_grad_norm_(1e30)
            o.step()
        o.join()
        torch.cuda.synchronize()
        res.append({k: v.detach().cpu().numpy().copy() for k, v in m.state_dict().items()})
    for k in res[0]:
        assert np.array_equal(res[0][k], res[1][k]), k


def test_clip_with_held_back_weight_gradients(monkeypatch):
    """deferral on (top 2 units held back): the norm includes them (computed at the clip call), each is applied once"""
    from oracle import w2l_oracle as O
    from wav2letter_pytorch_amd.optim import FusedSGD
    _bit_reproducible(monkeypatch)
    sd = O.init_wav2letter_state(LAYERS, seed=14)
    x, il, tg, tl = O.synthetic_batch(2, 160, seed=11, s_lo=5, s_hi=15)
    runs = []
    for defer in (2, 0):
        m = build_w2l(LAYERS, sd, 'bf16').train()
        o = FusedSGD.from_sgd(torch.optim.SGD(m.parameters(), **KW))
        o.overlap = True
        o.defer_wgrad(m, defer)
        norms, held = [], []
        for _ in range(3):
            o.zero_grad(set_to_none=True)
            out, ol = m(x.cuda(), il)
            m.criterion(out.transpose(0, 1), tg, ol, tl).backward()
            held.append(len(m.engine()._deferred))
            norms.append(float(o.clip_grad_norm_(1e-3)))
            assert not m.engine()._deferred
            o.step()
        o.join()
        runs.append((norms, held, {k: v.detach().cpu().numpy().copy() for k, v in m.named_parameters()}))
    assert runs[0][1] == [2, 2, 2] and runs[1][1] == [0, 0, 0]
    for a, b in zip(runs[0][0], runs[1][0]):
        assert abs(a - b) <= 1e-5 * b, (runs[0][0], runs[1][0])
    for k in runs[0][2]:
        assert scale_err(runs[0][2][k], runs[1][2][k]) < 2e-5, k


def _replay_run(steps, replay_on, change_at):
    from oracle import w2l_oracle as O
    from wav2letter_pytorch_amd import replay
    from wav2letter_pytorch_amd.optim import FusedSGD
    layers = [(128, 11, 2, 1, 0.0), (192, 13, 1, 1, 0.0), (128, 29, 1, 2, 0.0)]
    sd = O.init_wav2letter_state(layers, seed=41)
    batches = []
    for b in range(3):
        x, il, tg, tl = O.synthetic_batch(4, 300, seed=50 + b, s_lo=8, s_hi=30)
        batches.append((x.cuda(), il, tg.cuda(), tl.cuda()))
    replay.ENABLED = replay_on
    for k in ('recorded', 'replayed_F', 'replayed_B', 'replayed_O', 'replayed_X'):
        replay.STATS[k] = 0
    replay.STATS['poisoned'] = []
    try:
        torch.manual_seed(11)
        model = build_w2l(layers, sd, 'bf16').cuda().train()
        model.check_nan = False
        opt = FusedSGD.from_sgd(torch.optim.SGD(model.parameters(), lr=0.02, momentum=0.9, nesterov=True, weight_decay=1e-4))
        opt.overlap = True
        trace, norms = [], []
        for i in range(steps):
            x, il, tg, tl = batches[i % len(batches)]
            opt.zero_grad(set_to_none=True)
            out, ol = model(x, il)
            model.criterion(out.transpose(0, 1), tg, ol, tl).backward()
            norms.append(opt.clip_grad_norm_(0.05 if i < change_at else 0.02))
            opt.step()
            trace.append((replay.STATS['recorded'], replay.STATS['replayed_O']))
        opt.join()
        torch.cuda.synchronize()
        return ([float(n) for n in norms], {k: v.detach().cpu().numpy().copy() for k, v in model.state_dict().items()}, trace,
                list(replay.STATS['poisoned']))
    finally:
        replay.ENABLED = True


def test_clipped_steps_replay_bit_identical(monkeypatch):
    _bit_reproducible(monkeypatch)
    steps, change = 12, 8
    ne, pe, _, _ = _replay_run(steps, False, change)
    nr, pr, trace, poisoned = _replay_run(steps, True, change)
    assert poisoned == [], poisoned
    assert ne == nr
    for k in pe:
        assert np.array_equal(pe[k], pr[k]), k
    # steady state before the change (two replayed phases O in a row) and every step after it replayed: max_norm only reaches
    # the clip buffer, no new recording
    assert trace[change - 1][1] - trace[change - 3][1] == 2, trace
    assert trace[-1][1] - trace[change - 1][1] == steps - change, trace
    assert trace[-1][0] == trace[change - 1][0], trace


def test_novograd_generic_clip_matches_torch(monkeypatch):
    from oracle import w2l_oracle as O
    from wav2letter_pytorch_amd.novograd import Novograd
    from wav2letter_pytorch_amd.optim import clip_gradients
    _bit_reproducible(monkeypatch)
    sd = O.init_wav2letter_state(LAYERS, seed=8)
    x, il, tg, tl = O.synthetic_batch(2, 160, seed=13, s_lo=5, s_hi=15)
    res = []
    for ours in (True, False):
        m = build_w2l(LAYERS, sd, 'bf16').train()
        o = Novograd(m.parameters(), lr=0.01, betas=(0.95, 0.5), weight_decay=1e-3)
        norms = []
        for _ in range(3):
            o.zero_grad(set_to_none=True)
            out, ol = m(x.cuda(), il)
            m.criterion(out.transpose(0, 1), tg, ol, tl).backward()
            if ours:
                norms.append(float(clip_gradients(o, 1e-3, 'norm', model=m)))
            else:
                norms.append(float(torch.nn.utils.clip_grad_norm_(list(m.parameters()), 1e-3)))
            o.step()
        torch.cuda.synchronize()
        res.append((norms, {k: v.detach().cpu().numpy().copy() for k, v in m.named_parameters()}))
    assert res[0][0] == res[1][0]
    for k in res[0][1]:
        assert np.array_equal(res[0][1][k], res[1][1][k]), k


def _trainer_case():
    from oracle import w2l_oracle as O
    layers = [(128, 11, 2, 1, 0.0), (128, 11, 1, 1, 0.0), (128, 11, 1, 1, 0.0), (128, 11, 1, 1, 0.0)]
    sd = O.init_wav2letter_state(layers, seed=21)
    x, il, tg, tl = O.synthetic_batch(4, 200, seed=22, s_lo=5, s_hi=12)
    texts = tuple(''.join(O.ENGLISH_LOWERCASE[int(i)] for i in tg[n, :int(tl[n])]) for n in range(4))
    batch = (x, il, tg, tl, ('a', 'b', 'c', 'd'), texts)

    def make():
        m = build_w2l(layers, sd, 'bf16')
        m._cfg.optimizer.lr = 0.05
        return m
    return make, batch


def _hand_loop(make, batch, steps, clip):
    model = make().train()
    opt = model.configure_optimizers()[0][0]
    opt.overlap = True
    model._optimizers = opt                      # (what trainer.Trainer sets: training_step logs the learning rate)
    for i in range(steps):
        opt.zero_grad(set_to_none=True)
        loss = model.training_step(batch, i)
        loss.backward()
        opt.clip_grad_norm_(clip)
        opt.step()
        model.on_train_batch_end(loss, batch, i)
    opt.join()
    torch.cuda.synchronize()
    return {k: v.detach().cpu().numpy().copy() for k, v in model.named_parameters()}


def test_trainer_gradient_clip_val(tmp_path, monkeypatch):
    from wav2letter_pytorch_amd.trainer import Trainer
    monkeypatch.delenv('W2L_DEFER_WGRAD', raising=False)
    _bit_reproducible(monkeypatch)
    make, batch = _trainer_case()
    calls = []
    results = {}
    for clip in (None, 1e-2):
        model = make()
        hook = model.configure_gradient_clipping

        def counted(*a, _hook=hook, **k):
            calls.append(clip)
            return _hook(*a, **k)
        model.configure_gradient_clipping = counted
        tr = Trainer(default_root_dir=str(tmp_path), max_epochs=1, max_steps=4, enable_checkpointing=False, gradient_clip_val=clip)
        tr.fit(model, [batch] * 4)
        n_units = len(model.engine().units)
        assert model.engine().defer_wgrad == (min(4, n_units // 4) if clip is None else 0), (clip, n_units)
        results[clip] = {k: v.detach().cpu().numpy().copy() for k, v in model.named_parameters()}
    assert len(model.engine().units) >= 4
    assert calls == [1e-2] * 4                      # never called with clipping off, once per step with it on
    ref = _hand_loop(make, batch, 4, 1e-2)
    for k in ref:
        assert scale_err(results[1e-2][k], ref[k]) < 2e-5, k
    assert any(not np.array_equal(results[None][k], ref[k]) for k in ref)       # the clipping did something


def test_lightning_hook_both_signatures(monkeypatch):
    """a subprocess injects a minimal pytorch_lightning whose Trainer calls configure_gradient_clipping in Lightning's closure
    order (1.x and 2.x signatures): same parameters as the hand-written clipped loop; an unknown algorithm raises ValueError"""
    _bit_reproducible(monkeypatch)
    make, batch = _trainer_case()
    ref = _hand_loop(make, batch, 4, 1e-2)
    for sig in ('1', '2'):
        out = subprocess.run([sys.executable, os.path.join(HERE, 'lightning_clip_worker.py'), sig], capture_output=True, text=True,
                             timeout=280, env=dict(os.environ, W2L_DETERMINISTIC='1', W2L_FOLD_BN_FWD='0', W2L_FAST_BN_BWD='0'))
        assert out.returncode == 0, out.stderr[-3000:]
        d = json.loads([l for l in out.stdout.splitlines() if l.startswith('{')][-1])
        assert d['bad_algorithm_raises'] and d['hook_calls'] == 4 and d['zero_clip_noop'], d
        got = np.load(d['params'])
        for k in ref:
            assert scale_err(got[k], ref[k]) < 2e-5, (sig, k)


def test_data_parallel_one_rank_clipped_steps_match_single_process(tmp_path):
    import socket
    env = dict(os.environ, RANK='0', LOCAL_RANK='0', WORLD_SIZE='1', MASTER_ADDR='127.0.0.1')
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        env['MASTER_PORT'] = str(s.getsockname()[1])
    base = str(tmp_path / 'dp')
    out = subprocess.run([sys.executable, os.path.join(HERE, 'dp_clip_worker.py'), base], capture_output=True, text=True,
                         timeout=280, env=env)
    assert out.returncode == 0, out.stderr[-3000:]
    got = np.load(base + '.dp.npz')
    ref = np.load(base + '.single.npz')
    assert abs(float(got['norm']) - float(ref['norm'])) <= 1e-5 * float(ref['norm'])
    for k in ref.files:
        if k.startswith('p/'):
            assert scale_err(got[k], ref[k]) < 2e-5, k
