"""Fused Adam / AdamW on a real MI355X: w2l_adam_tick against its host model (tests/adam_refs.py tick_host), w2l_adam_pack and
w2l_adam_small_multi against the float64 reference under its derived per-element bound (adam_refs.adam_ref, pinned to torch in
tests/test_cpu_adam.py; the operand packs checked exactly as for w2l_sgd_pack), one real optimizer step teacher-forced
against the same reference, replayed steps under a learning rate that changes at EVERY step against the eager run bit for
bit -- with the optimizer phase recorded at most once per record set -- and the Trainer stepping a scheduler per batch."""
import os

import numpy as np
import pytest
import torch

import adam_refs as A
import kernel_refs as R
from direct_helpers import Buf, guards, last_error, p, ratio, record
from gpu_helpers import build_w2l
from test_gpu_kernels_direct import Q_SCALE, SGD_SHAPES, PackState, outputs

pytestmark = pytest.mark.gpu

B1, B2 = A.ADAM_BETAS
EPS = A.ADAM_EPS
LR = 1e-3
CLIP = (0.5, 0.25)


@pytest.fixture(scope='module')
def L():
    from wav2letter_pytorch_amd import _lib
    assert torch.cuda.is_available()
    return _lib


# ================================================================================================================================
# w2l_adam_tick
# ================================================================================================================================

STATE_DT = np.dtype([('step', '<i8'), ('pow1', '<f8'), ('pow2', '<f8')])


def _tick(L, n, lr, b1, b2):
    """n ticks on a fresh state -> (state as a host record, dyn as float32 [4]); guards checked"""
    host = np.zeros(1, dtype=STATE_DT)
    host['pow1'] = host['pow2'] = 1.0
    st = Buf((3,), torch.float64, torch.from_numpy(host.view(np.float64).copy()))
    dyn = Buf((4,))
    for _ in range(n):
        L.check(L.lib.w2l_adam_tick(p(L, st), p(L, dyn), lr, b1, b2, L.stream_ptr()))
    torch.cuda.synchronize()
    assert guards(st, dyn)
    return st.np().view(STATE_DT)[0], dyn.np()


_DYN = {}


def real_dyn(L, n, lr):
    """the dyn scalars of step n as the device itself forms them (cached: the 1000-tick one is shared by every case)"""
    if (n, lr) not in _DYN:
        _DYN[n, lr] = _tick(L, n, lr, B1, B2)[1]
    return _DYN[n, lr]


@pytest.mark.parametrize('betas', [(0.9, 0.999), (0.95, 0.5)])
@pytest.mark.parametrize('n', [1, 2, 3, 1000])
def test_adam_tick(L, n, betas):
    b1, b2 = betas
    lr = 3e-4
    state, dyn = _tick(L, n, lr, b1, b2)
    step, pow1, pow2, want = A.tick_host(n, lr, b1, b2)
    assert int(state['step']) == step
    assert float(state['pow1']).hex() == pow1.hex() and float(state['pow2']).hex() == pow2.hex()      # bit-equal
    assert dyn[0] == np.float32(lr) and dyn[3] == 0.0
    for i in (1, 2):
        w = np.float32(want[i])
        print(f'tick n={n} betas={betas} dyn[{i}]: device {dyn[i]!r} host {w!r}')
        assert abs(float(dyn[i]) - float(w)) <= float(np.spacing(w)), (i, dyn[i], w)


def test_adam_tick_argument_checks(L):
    st, dyn = Buf((3,), torch.float64), Buf((4,))
    sp = L.stream_ptr()
    for name, call in {'null state': lambda: L.lib.w2l_adam_tick(None, p(L, dyn), 1e-3, 0.9, 0.999, sp),
                       'null dyn': lambda: L.lib.w2l_adam_tick(p(L, st), None, 1e-3, 0.9, 0.999, sp),
                       'beta1 = 1': lambda: L.lib.w2l_adam_tick(p(L, st), p(L, dyn), 1e-3, 1.0, 0.999, sp),
                       'beta2 < 0': lambda: L.lib.w2l_adam_tick(p(L, st), p(L, dyn), 1e-3, 0.9, -0.1, sp)}.items():
        assert call() != 0, name
        assert last_error(L).startswith('adam_tick'), (name, last_error(L))
    torch.cuda.synchronize()
    assert bool(torch.isnan(st.flat).all()) and bool(torch.isnan(dyn.flat).all())


# ================================================================================================================================
# w2l_adam_pack
# ================================================================================================================================

def sprinkle_zeros(t, gen):
    """about 1 % exact zeros; no other element below 2^-40 in magnitude (no subnormal intermediate: the smallest product,
    (1 - beta2) g^2 >= 2^-10 2^-80, is far inside the normal range)"""
    t[torch.rand(t.shape, generator=gen) < 0.01] = 0.0
    small = (t != 0) & (t.abs() < 2.0 ** -40)
    t[small] = 2.0 ** -40
    return t


class AdamState(PackState):
    """PackState plus the second moment; g and v carry exact zeros"""

    def __init__(self, shape, seed, lo, q):
        super().__init__(shape, seed, lo, q)
        cout, cin, kw = shape
        gen = torch.Generator().manual_seed(1000 + seed)
        self.g0 = sprinkle_zeros(self.g0, gen)
        self.g.t.copy_(self.g0)
        self.v0 = sprinkle_zeros(torch.randn(kw, cout, cin, generator=gen) ** 2, gen)
        self.v = Buf((kw, cout, cin), init=self.v0)
        self.dyn = self.clip = None

    def bufs(self):
        return super().bufs() + [self.v, self.dyn, self.clip]

    def args(self, L, dyn, wd, decoupled, zero_grad, clip=None):
        cout, cin, kw = self.shape
        self.dyn = Buf((4,), init=torch.from_numpy(np.asarray(dyn, dtype=np.float32)))
        self.clip = None if clip is None else Buf((4,), init=torch.tensor([0.0, clip[0], clip[1], 0.0]))
        return [p(L, self.p), p(L, self.g), p(L, self.m), p(L, self.v), p(L, self.dyn), B1, B2, EPS, wd, decoupled, zero_grad,
                cout, cin, kw, p(L, self.fh), p(L, self.fl), p(L, self.dh), p(L, self.dl), p(L, self.fq), p(L, self.dq),
                Q_SCALE if self.fq is not None else 1.0, p(L, self.clip), L.stream_ptr()]

    def adam(self, L, dyn, wd, decoupled, zero_grad, clip=None):
        L.check(L.lib.w2l_adam_pack(*self.args(L, dyn, wd, decoupled, zero_grad, clip)))
        torch.cuda.synchronize()

    def compare(self, dyn, wd, decoupled, clip, what):
        P, M, V = A.adam_ref(self.p0.double().numpy(), self.g0.double().numpy(), self.m0.double().numpy(), self.v0.double().numpy(),
                             [float(x) for x in dyn], B1, B2, EPS, wd, decoupled, *(clip or (None, None)))
        rs = [ratio(self.p.np(), P.v, P.bound()), ratio(self.m.np(), M.v, M.bound()), ratio(self.v.np(), V.v, V.bound())]
        print(f'{what}: error / bound  p {rs[0]:.4f}  m {rs[1]:.4f}  v {rs[2]:.4f}')
        assert max(rs) <= 1, f'{what}: error / bound (p, m, v) = {rs}'
        assert np.isfinite(self.p.np()).all() and (self.v.np() >= 0).all()
        return max(rs)


# (decoupled, wd, zero_grad, lo pairs, e4m3, clip, step whose dyn a real tick supplies, lr)
ADAM_FLAG_SETS = [(0, 0.0, 0, 0, 0, None, 1, LR), (1, 1e-2, 1, 1, 1, None, 1000, LR), (0, 1e-2, 0, 1, 0, CLIP, 1, LR),
                  (1, 0.0, 1, 0, 1, CLIP, 1000, LR), (1, 1e-2, 0, 0, 0, None, 1, 0.0), (0, 1e-2, 1, 0, 0, CLIP, 1000, 0.0),
                  (0, 1e-2, 0, 0, 1, None, 1000, LR), (1, 1e-2, 0, 1, 0, CLIP, 1, LR)]


@pytest.mark.parametrize('shape', SGD_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_adam_pack(L, shape):
    worst = 0.0
    for i, (dec, wd, zg, lo, q, clip, step, lr) in enumerate(ADAM_FLAG_SETS):
        what = f'adam_pack {shape} decoupled={dec} wd={wd} zero_grad={zg} lo={lo} e4m3={q} clip={clip} step={step} lr={lr}'
        dyn = real_dyn(L, step, lr)
        S = AdamState(shape, 120 + i, lo, q)
        S.adam(L, dyn, wd, dec, zg, clip)
        worst = max(worst, S.compare(dyn, wd, dec, clip, what))
        if zg:
            assert not S.g.np().view(np.uint32).any(), what
        else:
            assert np.array_equal(S.g.np().view(np.uint32), S.g0.numpy().view(np.uint32)), what
        assert np.array_equal(S.dyn.np(), np.asarray(dyn, dtype=np.float32)), what
        if clip is not None:
            assert S.clip.np().tolist() == [0.0, np.float32(clip[0]), np.float32(clip[1]), 0.0]
        if lr == 0.0:                                               # dyn[0] = dyn[1] = 0: the weights stand still
            assert np.array_equal(S.p.np().view(np.uint32), S.p0.numpy().view(np.uint32)), what
        S.check_operands(what)                                      # (guards of every buffer, v / dyn / clip included)
    record('adam', f'adam_pack {shape}', worst)


@pytest.mark.parametrize('shape', SGD_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_adam_pack_identity_clip_is_bit_identical(L, shape):
    dyn = real_dyn(L, 1000, LR)
    for dec in (0, 1):
        base, same = AdamState(shape, 177, 1, 1), AdamState(shape, 177, 1, 1)
        base.adam(L, dyn, 1e-2, dec, 0)
        same.adam(L, dyn, 1e-2, dec, 0, clip=(1.0, float('inf')))
        for a, b in zip(outputs(base)[:-1], outputs(same)[:-2]):          # (every buffer but the dyn / clip scalars themselves)
            assert np.array_equal(a, b), 'coef = 1, bound = +inf must be bit-identical to clip = NULL'


def test_adam_pack_argument_checks(L):
    """each is refused by a W2L_CHECK_ARG in front of the launch: nonzero return, a message naming adam_pack, nothing written"""
    shape = (64, 64, 3)
    dyn = real_dyn(L, 1, LR)
    S = AdamState(shape, 300, 1, 1)
    base = S.args(L, dyn, 1e-2, 1, 0, CLIP)
    before = [b.flat.clone() for b in S.bufs() if b is not None]

    def changed(**kw):
        a = list(base)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return a

    cases = {'null p': changed(_0=None), 'null g': changed(_1=None), 'null m': changed(_2=None), 'null v': changed(_3=None),
             'null dyn': changed(_4=None), 'beta1 = 1': changed(_5=1.0), 'beta2 < 0': changed(_6=-0.5), 'eps < 0': changed(_7=-1e-8),
             'Cout = 0': changed(_11=0), 'Cin < 0': changed(_12=-64), 'Kw = 0': changed(_13=0),
             'fwd lo without hi': changed(_14=None, _18=None, _19=None), 'dgr lo without hi': changed(_16=None, _18=None, _19=None),
             'e4m3 without scale': changed(_20=0.0), 'e4m3 without bf16 operands': changed(_14=None, _15=None)}
    for name, args in cases.items():
        assert L.lib.w2l_adam_pack(*args) != 0, name
        assert last_error(L).startswith('adam_pack'), (name, last_error(L))
    torch.cuda.synchronize()
    for b, was in zip([b for b in S.bufs() if b is not None], before):
        assert torch.equal(b.flat.view(torch.uint8), was.view(torch.uint8)), 'a refused call wrote something'


# ================================================================================================================================
# w2l_adam_small_multi
# ================================================================================================================================

SMALL_N = [1, 255, 2048, 2049, 29 * 1024]


class SmallState:
    def __init__(self, seed):
        gen = torch.Generator().manual_seed(seed)
        self.items = []
        for n in SMALL_N:
            p0, m0 = torch.randn(n, generator=gen), torch.randn(n, generator=gen)
            g0 = sprinkle_zeros(torch.randn(n, generator=gen), gen)
            v0 = sprinkle_zeros(torch.randn(n, generator=gen) ** 2, gen)
            self.items.append(dict(n=n, p0=p0, g0=g0, m0=m0, v0=v0, p=Buf((n,), init=p0), g=Buf((n,), init=g0), m=Buf((n,), init=m0),
                                   v=Buf((n,), init=v0)))
        flat = []
        for it in self.items:
            flat += [it[k].t.data_ptr() for k in 'pgmv'] + [it['n']]
        self.table = Buf((len(flat),), torch.int64, torch.tensor(flat, dtype=torch.int64))

    def run(self, L, dyn, wd, decoupled, clip=None):
        self.dyn = Buf((4,), init=torch.from_numpy(np.asarray(dyn, dtype=np.float32)))
        self.clip = None if clip is None else Buf((4,), init=torch.tensor([0.0, clip[0], clip[1], 0.0]))
        L.check(L.lib.w2l_adam_small_multi(p(L, self.table), len(self.items), max(SMALL_N), p(L, self.dyn), B1, B2, EPS, wd, decoupled,
                                           p(L, self.clip), L.stream_ptr()))
        torch.cuda.synchronize()

    def compare(self, dyn, wd, decoupled, clip, what):
        worst = 0.0
        for it in self.items:
            P, M, V = A.adam_ref(*(it[k].double().numpy() for k in ('p0', 'g0', 'm0', 'v0')), [float(x) for x in dyn], B1, B2, EPS, wd,
                                 decoupled, *(clip or (None, None)))
            r = max(ratio(it['p'].np(), P.v, P.bound()), ratio(it['m'].np(), M.v, M.bound()), ratio(it['v'].np(), V.v, V.bound()))
            assert r <= 1, f'{what} item n={it["n"]}: error / bound = {r}'
            assert np.array_equal(it['g'].np().view(np.uint32), it['g0'].numpy().view(np.uint32)), 'the gradient is not written'
            assert guards(it['p'], it['g'], it['m'], it['v']), f'{what} item n={it["n"]}: guard touched'
            worst = max(worst, r)
        assert guards(self.table, self.dyn, self.clip)
        return worst


def test_adam_small_multi(L):
    d4 = torch.zeros(4, device='cuda')
    assert L.lib.w2l_adam_small_multi(None, 0, 0, L.ptr(d4), B1, B2, EPS, 0.0, 0, None, L.stream_ptr()) == 0
    assert L.lib.w2l_adam_small_multi(None, 1, 8, L.ptr(d4), B1, B2, EPS, 0.0, 0, None, L.stream_ptr()) != 0
    assert last_error(L).startswith('adam_small_multi')
    worst = 0.0
    for step in (1, 1000):
        dyn = real_dyn(L, step, LR)
        for dec, wd in ((0, 0.0), (0, 1e-2), (1, 1e-2)):
            for clip in (None, CLIP):
                S = SmallState(40 + step)
                S.run(L, dyn, wd, dec, clip)
                worst = max(worst, S.compare(dyn, wd, dec, clip, f'adam_small_multi step={step} decoupled={dec} wd={wd} clip={clip}'))
    base, same = SmallState(44), SmallState(44)
    base.run(L, real_dyn(L, 1000, LR), 1e-2, 1)
    same.run(L, real_dyn(L, 1000, LR), 1e-2, 1, clip=(1.0, float('inf')))
    for a, b in zip(base.items, same.items):
        for k in 'pmv':
            assert np.array_equal(a[k].np().view(np.uint32), b[k].np().view(np.uint32)), 'identity clip must be bit-identical'
    record('adam', 'adam_small_multi', worst)


# ================================================================================================================================
# optim.FusedAdamW: one real step, replayed steps, a parameter that misses a gradient
# ================================================================================================================================

LAYERS = [(128, 11, 2, 1, 0.0), (192, 13, 1, 1, 0.0), (128, 29, 1, 2, 0.0)]


def _bit_reproducible(monkeypatch):
    from wav2letter_pytorch_amd import engine as E
    monkeypatch.setattr(E, 'FOLD_BN_FWD', '0')
    monkeypatch.setattr(E, 'FAST_BN_BWD', False)
    monkeypatch.setattr(E, 'DETERMINISTIC_WGRAD', True)


_CASE = {}


def _w2l_case():
    """the 3-layer Wav2Letter of tests/test_gpu_replay.py (N = 4, T = 300), three batches"""
    if not _CASE:
        from oracle import w2l_oracle as O
        _CASE['sd'] = O.init_wav2letter_state(LAYERS, seed=41)
        _CASE['batches'] = []
        for b in range(3):
            x, il, tg, tl = O.synthetic_batch(4, 300, seed=50 + b, s_lo=8, s_hi=30)
            _CASE['batches'].append((x.cuda(), il, tg.cuda(), tl.cuda()))
    return (lambda: build_w2l(LAYERS, _CASE['sd'], 'bf16')), _CASE['batches']


def _host(t):
    return t.detach().cpu().double().numpy()


@pytest.mark.parametrize('cls,wd', [(torch.optim.AdamW, 1e-2), (torch.optim.Adam, 1e-3)])
def test_one_real_step_within_bound(cls, wd):
    """teacher-forced: p, g, m, v read back before step() at steps 1 and 3, every parameter afterwards within adam_ref's bound
    of THAT state, the reference fed the device's own dyn scalars"""
    from wav2letter_pytorch_amd.optim import FusedAdamW
    make, batches = _w2l_case()
    torch.manual_seed(11)
    model = make().cuda().train()
    model.check_nan = False
    opt = FusedAdamW.from_adam(cls(model.parameters(), lr=LR, betas=(B1, B2), eps=EPS, weight_decay=wd))
    opt.overlap = True
    names = {id(q): k for k, q in model.named_parameters()}
    worst = 0.0
    for step in (1, 2, 3):
        x, il, tg, tl = batches[step % 3]
        opt.zero_grad(set_to_none=True)
        out, ol = model(x, il)
        model.criterion(out.transpose(0, 1), tg, ol, tl).backward()
        opt.join()
        torch.cuda.synchronize()
        before = {}
        for q in model.parameters():
            st = opt.state.get(q, {})
            zero = np.zeros(tuple(q.shape))
            before[id(q)] = (_host(q), _host(q.grad), _host(st['exp_avg']) if 'exp_avg' in st else zero,
                             _host(st['exp_avg_sq']) if 'exp_avg_sq' in st else zero)
        opt.step()
        opt.join()
        torch.cuda.synchronize()
        if step == 2:
            continue
        dyn = opt._scalars(0)['dyn'].cpu().numpy()
        want = A.tick_host(step, LR, B1, B2)
        assert opt._scalars(0)['count'] == step and dyn[0] == np.float32(LR)
        assert abs(float(dyn[1]) - float(np.float32(want[3][1]))) <= float(np.spacing(np.float32(want[3][1])))
        for q in model.parameters():
            P, M, V = A.adam_ref(*before[id(q)], [float(v) for v in dyn], B1, B2, EPS, wd, int(cls is torch.optim.AdamW))
            st = opt.state[q]
            r = max(ratio(_host(q), P.v, P.bound()), ratio(_host(st['exp_avg']), M.v, M.bound()),
                    ratio(_host(st['exp_avg_sq']), V.v, V.bound()))
            assert r <= 1, f'step {step} {names[id(q)]}: error / bound = {r}'
            assert st['step'] == step
            worst = max(worst, r)
    record('adam', f'one real step {cls.__name__}', worst)


def _lr_lambda(s):
    """4 warm-up steps, then decay: a different learning rate at every step"""
    return (s + 1) / 4.0 if s < 4 else 0.9 ** (s - 3)


def _run(replay_on, steps, defer, clip, freeze_at=None):
    from wav2letter_pytorch_amd import _lib, replay
    from wav2letter_pytorch_amd.optim import FusedAdamW
    make, batches = _w2l_case()
    replay.ENABLED = replay_on
    _lib.AUDIT = replay_on
    for k in ('recorded', 'recorded_O', 'replayed_F', 'replayed_B', 'replayed_O', 'replayed_X'):
        replay.STATS[k] = 0
    replay.STATS['poisoned'] = []
    try:
        torch.manual_seed(11)
        model = make().cuda().train()
        model.check_nan = False
        opt = FusedAdamW.from_adam(torch.optim.AdamW(model.parameters(), lr=2e-3, betas=(B1, B2), eps=EPS, weight_decay=1e-2))
        opt.overlap = True
        sch = torch.optim.lr_scheduler.LambdaLR(opt, _lr_lambda)
        if defer:
            opt.defer_wgrad(model, defer)
        # (a BatchNorm bias: a conv bias in front of BatchNorm has a gradient of rounding noise only -- nothing to tell two
        # bias corrections apart by)
        frozen = model.conv1ds.conv1d_1.batch_norm.bias
        losses, lrs, seen, held_at_step = [], [], {}, []
        for i in range(steps):
            x, il, tg, tl = batches[i % len(batches)]
            opt.zero_grad(set_to_none=True)
            out, ol = model(x, il)
            loss = model.criterion(out.transpose(0, 1), tg, ol, tl)
            loss.backward()
            if freeze_at is not None and i >= freeze_at:
                opt.join()
                torch.cuda.synchronize()
                if i == freeze_at:
                    frozen.grad = None                           # this parameter misses ONE gradient
                else:
                    st = opt.state[frozen]
                    seen[i] = (_host(frozen), _host(frozen.grad), _host(st['exp_avg']), _host(st['exp_avg_sq']), st['step'],
                               opt.param_groups[0]['lr'])
            if clip:
                opt.clip_grad_norm_(clip)
            held_at_step.append(sum(len(eng._deferred) for eng in opt._engines()))
            lrs.append(opt.param_groups[0]['lr'])
            opt.step()
            sch.step()
            if i in seen:
                opt.join()
                torch.cuda.synchronize()
                seen[i] += (_host(frozen), opt.state[frozen]['step'])
            losses.append(float(loss))
        opt.join()
        torch.cuda.synchronize()
        params = {k: v.detach().cpu().numpy().copy() for k, v in model.state_dict().items()}
        stats = dict(replay.STATS, held_at_step=held_at_step)
        if replay_on:
            bad = replay.audit(model.engine())
            assert bad == [], bad[:8]
        return losses, params, stats, lrs, seen, opt
    finally:
        replay.ENABLED = True
        _lib.AUDIT = False


@pytest.mark.parametrize('clip', [None, 0.5], ids=['noclip', 'clip'])
@pytest.mark.parametrize('defer', [0, 2])
def test_replayed_adam_steps_equal_eager_steps(defer, clip, monkeypatch):
    """12 steps under a LambdaLR that changes the learning rate at every step: losses and final parameters of the replayed run
    equal the eager run's bit for bit, and the optimizer phase was recorded at most once per record set (two sets) although no
    two steps shared a learning rate.  With clipping armed the clip call computes every held-back gradient itself, so nothing
    is left for a phase X (optim.FusedBase.clip_grad_norm_): the phase-X condition applies where gradients are held back."""
    _bit_reproducible(monkeypatch)
    steps = 12
    le, pe, _, lrs, _, _ = _run(False, steps, defer, clip)
    lr_, pr, st, lrs_r, _, _ = _run(True, steps, defer, clip)
    print('replay statistics:', st)
    assert len(set(lrs)) == steps and lrs == lrs_r
    assert st['poisoned'] == [], st
    assert st['replayed_O'] >= 3, st
    if defer and not clip:
        assert st['held_at_step'][2:] == [defer] * (steps - 2), st   # step() found the top units' gradients held back
        assert st['replayed_X'] >= 2, st
    if defer and clip:
        # the clip call computed every held-back gradient (they belong in the norm): none left at step(), no phase X at all,
        # every weight updated in phase O
        assert st['held_at_step'] == [0] * steps and st['replayed_X'] == 0, st
    assert st['recorded_O'] <= 2, st
    assert le == lr_, (le, lr_)
    for k in pe:
        assert np.array_equal(pe[k], pr[k]), k


def test_parameter_that_missed_a_gradient_keeps_its_own_count(monkeypatch):
    """one (BatchNorm) bias misses the gradient of step 5 (of 9): from then on it is updated by torch's rule with ITS step count -- one
    behind the group's -- within the bound, never with the group's bias correction; the run completes, replay on"""
    _bit_reproducible(monkeypatch)
    losses, params, st, lrs, seen, opt = _run(True, 9, 0, None, freeze_at=4)
    assert len(losses) == 9 and all(np.isfinite(losses))
    assert sorted(seen) == [5, 6, 7, 8]
    for i, (p0, g0, m0, v0, step0, lr, p1, step1) in seen.items():
        assert step0 == i - 1 and step1 == i and opt._scalars(0)['count'] >= i + 1       # its own count, one behind
        own = [float(np.float32(x)) for x in A.tick_host(step1, lr, B1, B2)[3]]
        P, _, _ = A.adam_ref(p0, g0, m0, v0, own, B1, B2, EPS, 1e-2, 1, torch_scalars=True)
        # torch's ops form the step scalars in float64: the bound covers any order of the same fp32 operations, plus one
        # rounding of each of the two scalars to fp32 (a relative 2^-24 on the update each)
        slack = 2 * R.U * np.abs(P.v - p0)
        r = ratio(p1, P.v, P.bound() + slack)
        assert r <= 1, f'step {i}: error / bound = {r}'
        group = [float(np.float32(x)) for x in A.tick_host(i + 1, lr, B1, B2)[3]]
        Pg, _, _ = A.adam_ref(p0, g0, m0, v0, group, B1, B2, EPS, 1e-2, 1, torch_scalars=True)
        if i == 5:
            assert ratio(p1, Pg.v, Pg.bound() + slack) > 1, 'the group\'s bias correction would have passed too: the test shows nothing'


# ================================================================================================================================
# Trainer: a scheduler stepped per batch
# ================================================================================================================================

def test_trainer_steps_scheduler_per_batch_and_resumes(tmp_path, monkeypatch):
    from oracle import w2l_oracle as O
    from wav2letter_pytorch_amd.config import to_cfg
    from wav2letter_pytorch_amd.optim import FusedAdamW
    from wav2letter_pytorch_amd.trainer import Trainer
    monkeypatch.delenv('W2L_DEFER_WGRAD', raising=False)
    # (shapes no other test trains on: the kernel plans measured here are process-wide, and tests that compare a run in this
    # process with one in a fresh process must find the plan tables as they would without this test)
    layers = [(192, 9, 2, 1, 0.0), (192, 9, 1, 1, 0.0)]
    sd = O.init_wav2letter_state(layers, seed=21)
    sched = dict(_target_='torch.optim.lr_scheduler.OneCycleLR', max_lr=2e-3, total_steps=20, pct_start=0.25, cycle_momentum=False)

    def make():
        m = build_w2l(layers, sd, 'bf16')
        m._cfg.optimizer = to_cfg(dict(_target_='torch.optim.AdamW', lr=1e-3, weight_decay=1e-2))
        m._cfg.scheduler = to_cfg(sched)
        m._cfg.scheduler_interval = 'step'
        return m

    x, il, tg, tl = O.synthetic_batch(3, 180, seed=22, s_lo=5, s_hi=12)
    texts = tuple(''.join(O.ENGLISH_LOWERCASE[int(i)] for i in tg[n, :int(tl[n])]) for n in range(3))
    batch = (x, il, tg, tl, ('a', 'b', 'c'), texts)
    dummy = torch.optim.AdamW([torch.nn.Parameter(torch.zeros(1))], lr=1e-3)
    ref_s = torch.optim.lr_scheduler.OneCycleLR(dummy, max_lr=2e-3, total_steps=20, pct_start=0.25, cycle_momentum=False)
    want = []
    for _ in range(16):
        want.append(dummy.param_groups[0]['lr'])
        dummy.step()
        ref_s.step()
    model = make()
    tr = Trainer(default_root_dir=str(tmp_path), max_epochs=1, log_every_n_steps=1)
    tr.fit(model, [batch] * 8)
    assert isinstance(model._optimizers, FusedAdamW)
    assert [s for s, _ in tr.logged] == list(range(1, 9))
    got = [l['learning_rate'] for _, l in tr.logged]
    assert got == pytest.approx(want[:8], rel=1e-12), (got, want[:8])
    assert len(set(got)) == 8
    ck = [f for f in sorted(os.listdir(tmp_path)) if f.endswith('.ckpt')]
    assert len(ck) == 1
    saved = torch.load(os.path.join(tmp_path, ck[0]))
    assert saved['lr_schedulers'][0]['last_epoch'] == 8 and saved['global_step'] == 8
    assert float(saved['optimizer_states'][0]['state'][0]['step']) == 8.0
    model2 = make()
    tr2 = Trainer(default_root_dir=str(tmp_path / 'resumed'), max_epochs=2, log_every_n_steps=1,
                  resume_from_checkpoint=os.path.join(tmp_path, ck[0]))
    tr2.fit(model2, [batch] * 8)
    assert [s for s, _ in tr2.logged] == list(range(9, 17))
    got2 = [l['learning_rate'] for _, l in tr2.logged]
    assert got2 == pytest.approx(want[8:], rel=1e-12), (got2, want[8:])
    assert model2._optimizers._scalars(0)['count'] == 16
