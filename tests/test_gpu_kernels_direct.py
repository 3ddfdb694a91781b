"""The depthwise-convolution, fused-optimizer and pad-cast entry points called directly, each against its float64 reference
(tests/kernel_refs.py, itself pinned by tests/test_cpu_kernel_refs.py) under a derived per-element bound:

    |got - ref| <= (n_terms + 2) u A + r_out,    u = 2^-24, A = the reference's sum of |term|,
    r_out = 0 (fp32 output), 2^-8 |ref| (bf16), 2^-17 |ref| (hi+lo pair)

Inputs are bf16 values or fp32 as given, so the reference is exact and the bound holds for any summation order and any FMA
contraction (the derivation is the docstring of kernel_refs.py).  Every output element is compared; output buffers start
as NaN (0xA5 bytes for e4m3) so an element the kernel must write and does not shows; every buffer is followed by a guard
region that must come back untouched.  Each test prints and asserts its worst error / bound ratio (must be <= 1)."""
import functools

import numpy as np
import pytest
import torch

import kernel_refs as R
from direct_helpers import Buf, guards, last_error, p, ratio, record

pytestmark = pytest.mark.gpu

SENTINEL = 1e4            # rows the kernels must never read
INF = float('inf')


@pytest.fixture(scope='module')
def L():
    from wav2letter_pytorch_amd import _lib
    assert torch.cuda.is_available()
    return _lib


# ================================================================================================================================
# depthwise convolution
# ================================================================================================================================

def big(shape):
    N, Tout, Cc = shape[:3]
    return N * Tout * Cc > (1 << 20)


@functools.lru_cache(maxsize=None)
def dw_data(shape):
    """host inputs of one shape: x as a bf16 value and as a hi+lo pair (both followed by sentinel rows), fp32 weights,
    dy as bf16 values and as fp32, each with 7 sentinel rows behind the Tout valid ones"""
    N, Tout, Cc, K, s, d = shape
    g = torch.Generator().manual_seed(100 + Cc + K)
    need = (Tout - 1) * s + (K - 1) * d + 1
    rows = need + 3
    x = torch.randn(N, rows, Cc, generator=g)
    x[:, need:] = SENTINEL
    hi = x.bfloat16()
    lo = (x - hi.float()).bfloat16()
    lo[:, need:] = 0
    w = torch.randn(K, Cc, generator=g)
    dy = torch.randn(N, Tout + 7, Cc, generator=g)
    dy[:, Tout:] = SENTINEL
    return dict(need=need, rows=rows, hi=hi, lo=lo, w=w, dy32=dy, dy16=dy.bfloat16())


def dw_x(shape, with_lo):
    D = dw_data(shape)
    v = D['hi'].double()
    return (v + D['lo'].double()) if with_lo else v


@functools.lru_cache(maxsize=None)
def dw_fwd_reference(shape, with_lo, kind):
    N, Tout, Cc, K, s, d = shape
    return R.dw_fwd_ref(dw_x(shape, with_lo).numpy(), dw_data(shape)['w'].double().numpy(), N, Tout, Cc, K, s, d,
                        R.dw_lens(kind, N, Tout))


def dev_lens(kind, N, Tout):
    lens = R.dw_lens(kind, N, Tout)
    return None if lens is None else Buf((N,), torch.int32, lens)


@pytest.mark.parametrize('shape', R.DW_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_dwconv_fwd(L, shape):
    N, Tout, Cc, K, s, d = shape
    D = dw_data(shape)
    xh, xl, w = Buf(D['hi'].shape, torch.bfloat16, D['hi']), Buf(D['lo'].shape, torch.bfloat16, D['lo']), Buf((K, Cc), init=D['w'])
    full = [(a, b, k) for k in R.LENS_KINDS for a in (0, 1) for b in (0, 1)]
    cover = [(0, 0, 'none'), (1, 1, 'full'), (0, 1, 'ragged'), (1, 0, 'over')]      # (16.8 M elements: the float64 reference takes ~1 s)
    worst = 0.0
    for with_lo, y_lo, kind in (cover if big(shape) else full):
        lens = dev_lens(kind, N, Tout)
        yh = Buf((N, Tout, Cc), torch.bfloat16)
        yl = Buf((N, Tout, Cc), torch.bfloat16) if y_lo else None
        L.check(L.lib.w2l_dwconv_fwd(p(L, xh), p(L, xl) if with_lo else None, D['rows'], p(L, w), p(L, yh), p(L, yl), N, Tout, Cc, K,
                                     s, d, p(L, lens), L.stream_ptr()))
        torch.cuda.synchronize()
        ref, A = dw_fwd_reference(shape, with_lo, kind)
        r = ratio(yh.np(), ref, R.dot_bound(A, K, ref, R.R_BF16))
        if yl is not None:
            r = max(r, ratio(yh.np().astype(np.float64) + yl.np(), ref, R.dot_bound(A, K, ref, R.R_SPLIT)))
        worst = max(worst, r)
        assert guards(xh, xl, w, yh, yl, lens), (with_lo, y_lo, kind)
        assert r <= 1, f'dwconv_fwd {shape} x_lo={with_lo} y_lo={y_lo} lens={kind}: error / bound = {r}'
        lims = R._lims(N, Tout, R.dw_lens(kind, N, Tout))
        for n in range(N):
            assert not yh.t[n, lims[n]:].float().abs().sum().item(), 'rows t >= lens[n] must be exactly zero'
    record('depthwise', f'fwd {shape}', worst)


DGRAD_SHAPES = [sh for sh in R.DW_SHAPES if sh[4] == 1]


@pytest.mark.parametrize('shape', DGRAD_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_dwconv_dgrad(L, shape):
    N, Tout, Cc, K, s, d = shape
    D = dw_data(shape)
    w = Buf((K, Cc), init=D['w'])
    w64 = D['w'].double().numpy()
    span = Tout + (K - 1) * d
    full = [(gf, of, ex, tp, k) for k in R.LENS_KINDS for gf in (0, 1) for of in (0, 1) for ex in (0, 7) for tp in (0, 5)]
    cover = [(0, 0, 0, 0, 'none'), (1, 1, 7, 5, 'full'), (0, 1, 7, 0, 'ragged'), (1, 0, 0, 5, 'over')]
    worst = 0.0
    refs = {}
    for gf, of, extra, tpx, kind in (cover if big(shape) else full):
        dy_rows, Tp = Tout + extra, span + tpx
        src = D['dy32'] if gf else D['dy16']
        dy = Buf((N, dy_rows, Cc), src.dtype, src[:, :dy_rows])
        lens = dev_lens(kind, N, Tout)
        dx = Buf((N, Tp, Cc), torch.float32 if of else torch.bfloat16)
        L.check(L.lib.w2l_dwconv_dgrad(p(L, dy), gf, dy_rows, p(L, w), p(L, dx), of, N, Tp, Tout, Cc, K, d, p(L, lens),
                                       L.stream_ptr()))
        torch.cuda.synchronize()
        key = (gf, Tp, kind)
        if key not in refs:
            refs[key] = R.dw_dgrad_ref(src[:, :Tout].double().numpy(), w64, N, Tp, Tout, Cc, K, d, R.dw_lens(kind, N, Tout))
        ref, A = refs[key]
        r = ratio(dx.np(), ref, R.dot_bound(A, K, ref, 0.0 if of else R.R_BF16))
        worst = max(worst, r)
        assert guards(dy, w, dx, lens)
        assert r <= 1, f'dwconv_dgrad {shape} dy_f32={gf} dxp_f32={of} dy_rows=Tout+{extra} Tp=span+{tpx} lens={kind}: error / bound = {r}'
    record('depthwise', f'dgrad {shape}', worst)


@pytest.mark.parametrize('shape', R.DW_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_dwconv_wgrad(L, shape):
    """n_terms = the number of valid (n, t) rows: however the rows are dealt to threads, LDS partials and atomics, one
    product passes through fewer rounding additions than there are non-zero terms, plus the one onto the prefilled dw"""
    N, Tout, Cc, K, s, d = shape
    D = dw_data(shape)
    xh, xl = Buf(D['hi'].shape, torch.bfloat16, D['hi']), Buf(D['lo'].shape, torch.bfloat16, D['lo'])
    full = [(gf, ex, k, 'zero') for k in R.LENS_KINDS for gf in (0, 1) for ex in (0, 7)]
    cover = [(0, 7, 'ragged', 'zero'), (1, 0, 'full', 'zero')]
    worst = 0.0
    g = torch.Generator().manual_seed(9)
    pre = torch.randn(K, Cc, generator=g) * 8
    tail = [(1, 0, 'over', 'random')] if big(shape) else [(1, 7, 'ragged', 'random'), (0, 0, 'none', 'random')]
    for i, (gf, extra, kind, fill) in enumerate((cover if big(shape) else full) + tail):
        with_lo = i % 2
        dy_rows = Tout + extra
        src = D['dy32'] if gf else D['dy16']
        dy = Buf((N, dy_rows, Cc), src.dtype, src[:, :dy_rows])
        lens = dev_lens(kind, N, Tout)
        dw = Buf((K, Cc), init=pre if fill == 'random' else torch.zeros(K, Cc))
        L.check(L.lib.w2l_dwconv_wgrad(p(L, dy), gf, dy_rows, p(L, xh), p(L, xl) if with_lo else None, D['rows'], p(L, dw), N, Tout, Cc,
                                       K, s, d, p(L, lens), L.stream_ptr()))
        torch.cuda.synchronize()
        ref, A, nt = R.dw_wgrad_ref(src[:, :Tout].double().numpy(), dw_x(shape, with_lo).numpy(), N, Tout, Cc, K, s, d,
                                    R.dw_lens(kind, N, Tout))
        if fill == 'random':
            ref, A = ref + pre.double().numpy(), A + pre.double().abs().numpy()
        r = ratio(dw.np(), ref, R.dot_bound(A, nt, ref))
        worst = max(worst, r)
        assert guards(dy, xh, xl, dw, lens)
        assert r <= 1, f'dwconv_wgrad {shape} dy_f32={gf} dy_rows=Tout+{extra} lens={kind} x_lo={with_lo} dw={fill}: error / bound = {r}'
    record('depthwise', f'wgrad {shape}', worst)


def test_dwconv_argument_checks(L):
    """each is refused by a W2L_CHECK_ARG in front of the launch: nonzero return, a message, the outputs untouched"""
    N, Tout, K = 2, 16, 3
    x = Buf((N, Tout + K - 1, 4096), torch.bfloat16, torch.zeros(N, Tout + K - 1, 4096))
    y = Buf((N, Tout + K - 1, 4096), torch.bfloat16)
    f = Buf((N, Tout + K - 1, 4096))
    w = Buf((K, 4096), init=torch.zeros(K, 4096))
    sp = L.stream_ptr()
    calls = {
        'fwd C%8': lambda: L.lib.w2l_dwconv_fwd(p(L, x), None, Tout + K - 1, p(L, w), p(L, y), None, N, Tout, 12, K, 1, 1, None, sp),
        'dgrad C%8': lambda: L.lib.w2l_dwconv_dgrad(p(L, x), 0, Tout, p(L, w), p(L, y), 0, N, Tout + K - 1, Tout, 12, K, 1, None, sp),
        'wgrad C%8': lambda: L.lib.w2l_dwconv_wgrad(p(L, x), 0, Tout, p(L, x), None, Tout + K - 1, p(L, f), N, Tout, 12, K, 1, 1, None, sp),
        'wgrad C>2048': lambda: L.lib.w2l_dwconv_wgrad(p(L, x), 0, Tout, p(L, x), None, Tout + K - 1, p(L, f), N, Tout, 2056, K, 1, 1,
                                                       None, sp),
        'fwd short input': lambda: L.lib.w2l_dwconv_fwd(p(L, x), None, Tout + K - 2, p(L, w), p(L, y), None, N, Tout, 64, K, 1, 1, None, sp),
        'wgrad short input': lambda: L.lib.w2l_dwconv_wgrad(p(L, x), 0, Tout, p(L, x), None, Tout + K - 2, p(L, f), N, Tout, 64, K, 1, 1,
                                                            None, sp),
        'dgrad Tout>dy_rows': lambda: L.lib.w2l_dwconv_dgrad(p(L, x), 0, Tout - 1, p(L, w), p(L, y), 0, N, Tout + K - 1, Tout, 64, K, 1,
                                                             None, sp),
        'wgrad Tout>dy_rows': lambda: L.lib.w2l_dwconv_wgrad(p(L, x), 0, Tout - 1, p(L, x), None, Tout + K - 1, p(L, f), N, Tout, 64, K, 1,
                                                             1, None, sp),
    }
    for name, call in calls.items():
        assert call() != 0, name
        assert last_error(L).startswith('dwconv_'), (name, last_error(L))
    torch.cuda.synchronize()
    assert bool(torch.isnan(y.flat).all()) and bool(torch.isnan(f.flat).all())


# ================================================================================================================================
# w2l_sgd_pack / w2l_sgd_pack_clip
# ================================================================================================================================

Q_SCALE = 112.5           # |p| beyond 448 / 112.5 ~ 3.98 saturates: the clamp of the e4m3 conversion is exercised too
SGD_SHAPES = [(64, 64, 1), (128, 64, 11), (192, 320, 3), (96, 40, 5)]


def e4m3_model(p32, scale):
    """tests/test_gpu_fp8.py's host model, applied to bf16(p) * q_scale"""
    v = torch.from_numpy(np.ascontiguousarray(p32)).bfloat16().float() * scale
    return v.clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8).numpy()


class PackState:
    """p / g / m in the dense tap-major [Kw][Cout][Cin] storage the optimizer passes, and the operand buffers"""

    def __init__(self, shape, seed, lo, q, m_nan=False, nan_at=None):
        cout, cin, kw = shape
        gen = torch.Generator().manual_seed(seed)
        self.shape = shape
        self.p0, self.g0, self.m0 = (torch.randn(kw, cout, cin, generator=gen) for _ in range(3))
        if nan_at is not None:
            self.g0.view(-1)[nan_at] = float('nan')
        self.p, self.g = Buf((kw, cout, cin), init=self.p0), Buf((kw, cout, cin), init=self.g0)
        self.m = Buf((kw, cout, cin), init=None if m_nan else self.m0)
        self.fh, self.dh = Buf((kw, cout, cin), torch.bfloat16), Buf((kw, cin, cout), torch.bfloat16)
        self.fl = Buf((kw, cout, cin), torch.bfloat16) if lo else None
        self.dl = Buf((kw, cin, cout), torch.bfloat16) if lo else None
        self.fq = Buf((kw, cout, cin), torch.uint8) if q else None
        self.dq = Buf((kw, cin, cout), torch.uint8) if q else None

    def bufs(self):
        return [self.p, self.g, self.m, self.fh, self.dh, self.fl, self.dl, self.fq, self.dq]

    def sgd(self, L, first, nesterov, wd, zero_grad, clip=None):
        cout, cin, kw = self.shape
        args = (p(L, self.p), p(L, self.g), p(L, self.m), first, R.SGD_LR, R.SGD_MU, wd, nesterov, zero_grad, cout, cin, kw,
                p(L, self.fh), p(L, self.fl), p(L, self.dh), p(L, self.dl), p(L, self.fq), p(L, self.dq),
                Q_SCALE if self.fq is not None else 1.0)
        if clip is None:
            L.check(L.lib.w2l_sgd_pack(*args, L.stream_ptr()))
        else:
            self.clip = Buf((4,), init=torch.tensor([0.0, clip[0], clip[1], 0.0]))
            L.check(L.lib.w2l_sgd_pack_clip(*args, p(L, self.clip), L.stream_ptr()))
        torch.cuda.synchronize()

    def check_operands(self, what):
        """the operands against the device's OWN updated p: hi bit-equal to bf16_rne(p) in both layouts, hi+lo within 2^-17,
        the e4m3 bytes bit-equal to the host model"""
        pd = self.p.np()
        pdT = np.ascontiguousarray(pd[::-1].transpose(0, 2, 1))           # [Kw-1-kw][Cin][Cout]
        for lay, hi, lo, q in ((pd, self.fh, self.fl, self.fq), (pdT, self.dh, self.dl, self.dq)):
            assert np.array_equal(hi.bits(), R.bf16_rne(lay)), what
            if lo is not None:
                rec = hi.np().astype(np.float64) + lo.np()
                assert (np.abs(rec - lay) <= R.R_SPLIT * np.abs(lay)).all(), what
                assert np.array_equal(lo.bits(), R.split_bf16(lay)[1]), what
            if q is not None:
                assert np.array_equal(q.np(), e4m3_model(lay, Q_SCALE)), what
        assert guards(*self.bufs()), what


@pytest.mark.parametrize('shape', SGD_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_sgd_pack(L, shape):
    worst = 0.0
    for i, (first, nesterov, wd, zg, lo, q) in enumerate(R.SGD_FLAG_SETS):
        what = f'sgd_pack {shape} first={first} nesterov={nesterov} wd={wd} zero_grad={zg} lo={lo} e4m3={q}'
        S = PackState(shape, 20 + i, lo, q, m_nan=bool(first))
        S.sgd(L, first, nesterov, wd, zg)
        P, M = R.sgd_ref(S.p0.double().numpy(), S.g0.double().numpy(), S.m0.double().numpy(), first, R.SGD_LR, R.SGD_MU, wd, nesterov)
        r = max(ratio(S.p.np(), P.v, P.bound()), ratio(S.m.np(), M.v, M.bound()))
        worst = max(worst, r)
        assert r <= 1, f'{what}: error / bound = {r}'
        assert np.isfinite(S.m.np()).all()
        if zg:
            assert not S.g.np().view(np.uint32).any(), what
        else:
            assert np.array_equal(S.g.np().view(np.uint32), S.g0.numpy().view(np.uint32)), what
        S.check_operands(what)
    record('sgd', f'sgd_pack {shape}', worst)


def outputs(S):
    return [b.flat.view(torch.uint8 if b.flat.dtype == torch.uint8 else (torch.int32 if b.flat.dtype == torch.float32 else torch.int16))
            .cpu().numpy() for b in S.bufs() if b is not None]


@pytest.mark.parametrize('shape', SGD_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_sgd_pack_clip(L, shape):
    first, nesterov, wd, zg = 0, 1, 1e-3, 0
    base = PackState(shape, 77, 1, 1)
    base.sgd(L, first, nesterov, wd, zg)
    same = PackState(shape, 77, 1, 1)
    same.sgd(L, first, nesterov, wd, zg, clip=(1.0, INF))
    for a, b in zip(outputs(base), outputs(same)):
        assert np.array_equal(a, b), 'coef = 1, bound = +inf must be bit-identical to w2l_sgd_pack'
    worst = 0.0
    for clip in R.SGD_CLIPS[1:]:
        for nest, zg2 in ((1, 1), (0, 0)):
            S = PackState(shape, 78, 0, 0)
            S.sgd(L, first, nest, wd, zg2, clip=clip)
            P, M = R.sgd_ref(S.p0.double().numpy(), S.g0.double().numpy(), S.m0.double().numpy(), first, R.SGD_LR, R.SGD_MU, wd, nest, *clip)
            r = max(ratio(S.p.np(), P.v, P.bound()), ratio(S.m.np(), M.v, M.bound()))
            worst = max(worst, r)
            assert r <= 1, f'sgd_pack_clip {shape} clip={clip} nesterov={nest}: error / bound = {r}'
            S.check_operands(f'sgd_pack_clip {shape} {clip}')
            assert guards(S.clip) and S.clip.np().tolist() == [0.0, np.float32(clip[0]), np.float32(clip[1]), 0.0]
    # a NaN gradient element poisons exactly its own p / m element
    n = base.p.n
    at = n - 7
    for clip in [None] + R.SGD_CLIPS:
        S = PackState(shape, 79, 0, 0, nan_at=at)
        S.sgd(L, first, nesterov, wd, zg, clip=clip)
        for out in (S.p.np(), S.m.np()):
            assert np.flatnonzero(np.isnan(out.ravel())).tolist() == [at], f'sgd_pack {shape} clip={clip}: NaN must stay where it was'
    record('sgd', f'sgd_pack_clip {shape}', worst)


# ================================================================================================================================
# w2l_sgd_small_multi / _clip
# ================================================================================================================================

SMALL_N = [1, 255, 256, 2047, 2048, 2049, 29 * 1024]
SMALL_NO_M = [300, 2049]


class SmallState:
    def __init__(self, seed, nan_at=None):
        gen = torch.Generator().manual_seed(seed)
        self.items = []
        for n in SMALL_N + SMALL_NO_M:
            p0, g0, m0 = (torch.randn(n, generator=gen) for _ in range(3))
            if nan_at is not None and n == 2049:
                g0[nan_at] = float('nan')
            has_m = len(self.items) < len(SMALL_N)
            self.items.append(dict(n=n, p0=p0, g0=g0, m0=m0 if has_m else None, p=Buf((n,), init=p0), g=Buf((n,), init=g0),
                                   m=Buf((n,), init=m0) if has_m else None))
        flat = []
        for it in self.items:
            flat += [it['p'].t.data_ptr(), it['g'].t.data_ptr(), it['m'].t.data_ptr() if it['m'] is not None else 0, it['n']]
        self.table = Buf((len(flat),), torch.int64, torch.tensor(flat, dtype=torch.int64))

    def run(self, L, nesterov, wd, clip=None):
        n, mx = len(self.items), max(it['n'] for it in self.items)
        if clip is None:
            L.check(L.lib.w2l_sgd_small_multi(p(L, self.table), n, mx, R.SGD_LR, R.SGD_MU, wd, nesterov, L.stream_ptr()))
        else:
            self.clip = Buf((4,), init=torch.tensor([0.0, clip[0], clip[1], 0.0]))
            L.check(L.lib.w2l_sgd_small_multi_clip(p(L, self.table), n, mx, R.SGD_LR, R.SGD_MU, wd, nesterov, p(L, self.clip),
                                                   L.stream_ptr()))
        torch.cuda.synchronize()

    def compare(self, nesterov, wd, clip, what):
        worst = 0.0
        for it in self.items:
            m0 = None if it['m0'] is None else it['m0'].double().numpy()
            P, M = R.sgd_ref(it['p0'].double().numpy(), it['g0'].double().numpy(), m0, 0, R.SGD_LR, R.SGD_MU, wd, nesterov,
                             *(clip or (None, None)))
            r = ratio(it['p'].np(), P.v, P.bound())
            if M is not None:
                r = max(r, ratio(it['m'].np(), M.v, M.bound()))
            assert r <= 1, f'{what} item n={it["n"]} m={"yes" if M is not None else "null"}: error / bound = {r}'
            assert np.array_equal(it['g'].np().view(np.uint32), it['g0'].numpy().view(np.uint32)), 'the gradient is not written'
            assert guards(it['p'], it['g'], it['m']), f'{what} item n={it["n"]}: guard touched'
            worst = max(worst, r)
        assert guards(self.table)
        return worst


def test_sgd_small_multi(L):
    assert L.lib.w2l_sgd_small_multi(None, 0, 0, 0.1, 0.9, 0.0, 0, L.stream_ptr()) == 0
    assert L.lib.w2l_sgd_small_multi_clip(None, 0, 0, 0.1, 0.9, 0.0, 0, L.ptr(torch.zeros(4, device='cuda')), L.stream_ptr()) == 0
    worst = 0.0
    for nesterov in (0, 1):
        for wd in (0.0, 1e-3):
            base = SmallState(40)
            base.run(L, nesterov, wd)
            worst = max(worst, base.compare(nesterov, wd, None, f'sgd_small_multi nesterov={nesterov} wd={wd}'))
            same = SmallState(40)
            same.run(L, nesterov, wd, clip=(1.0, INF))
            for a, b in zip(base.items, same.items):
                for k in ('p', 'm'):
                    if a[k] is not None:
                        assert np.array_equal(a[k].np().view(np.uint32), b[k].np().view(np.uint32)), 'identity clip must be bit-identical'
            for clip in R.SGD_CLIPS[1:]:
                S = SmallState(41)
                S.run(L, nesterov, wd, clip=clip)
                worst = max(worst, S.compare(nesterov, wd, clip, f'sgd_small_multi_clip nesterov={nesterov} wd={wd} clip={clip}'))
    for clip in [None] + R.SGD_CLIPS:
        S = SmallState(42, nan_at=2048)
        S.run(L, 1, 1e-3, clip=clip)
        for it in S.items:
            for k in ('p', 'm'):
                if it[k] is not None:
                    want = [2048] if it['n'] == 2049 else []
                    assert np.flatnonzero(np.isnan(it[k].np())).tolist() == want, f'clip={clip} n={it["n"]} {k}'
    record('sgd', 'sgd_small_multi', worst)


# ================================================================================================================================
# w2l_novograd_pack
# ================================================================================================================================

NOVO_SHAPES = [(64, 64, 1), (128, 64, 11), (96, 40, 5), (1024, 1024, 5)]      # (96, 40, 5): partial 32x32 tiles on both axes
NOVO = dict(lr=0.02, b1=0.95, b2=0.5, eps=1e-8)


def novo_step(L, S, gnew, v, vmax, scratch_floats, wd, ga, what):
    """one w2l_novograd_pack call on PackState ``S`` (its p and m as they are on the device), a fresh gradient, the given
    exp_avg_sq / max_exp_avg_sq; compared with novograd_ref on the same inputs.  Returns (ratio of p / m, of v / vmax)."""
    cout, cin, kw = S.shape
    n = cout * cin * kw
    p_in, m_in = S.p.np().astype(np.float64), S.m.np().astype(np.float64)
    S.g = Buf((kw, cout, cin), init=gnew)
    vb = Buf((1,), init=torch.tensor([v], dtype=torch.float32))
    vm = None if vmax is None else Buf((1,), init=torch.tensor([vmax], dtype=torch.float32))
    scratch = Buf((scratch_floats,))
    L.check(L.lib.w2l_novograd_pack(p(L, S.p), p(L, S.g), p(L, S.m), p(L, vb), p(L, vm), p(L, scratch), scratch_floats, NOVO['lr'],
                                    NOVO['b1'], NOVO['b2'], NOVO['eps'], wd, ga, cout, cin, kw, p(L, S.fh), p(L, S.fl), p(L, S.dh),
                                    p(L, S.dl), L.stream_ptr()))
    torch.cuda.synchronize()
    nb = R.novograd_nblocks(n, scratch_floats)
    P, M, V, VM = R.novograd_ref(p_in, gnew.double().numpy(), m_in, float(np.float32(v)), None if vmax is None else float(np.float32(vmax)),
                                 NOVO['lr'], NOVO['b1'], NOVO['b2'], NOVO['eps'], wd, ga, R.novograd_norm_depth(n, nb))
    rv = ratio(vb.np(), V.v, V.bound())
    if VM is not None:
        rv = max(rv, ratio(vm.np(), VM.v, VM.bound()))
    rp = max(ratio(S.p.np(), P.v, P.bound()), ratio(S.m.np(), M.v, M.bound()))
    assert rv <= 1, f'{what}: v / vmax error / bound = {rv}'
    assert rp <= 1, f'{what}: p / m error / bound = {rp}'
    assert np.array_equal(S.g.np().view(np.uint32), gnew.numpy().view(np.uint32)), 'the gradient is not written'
    assert not np.isnan(scratch.np()[:1 + nb]).any() and np.isnan(scratch.np()[1 + nb:]).all(), 'scratch: [denom | nblocks partials]'
    S.check_operands(what)
    assert guards(vb, vm, scratch), what
    return rp, rv, float(vb.np()[0])


@pytest.mark.parametrize('shape', NOVO_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_novograd_pack(L, shape):
    cout, cin, kw = shape
    huge = cout * cin * kw > (1 << 22)
    gen = torch.Generator().manual_seed(55)
    fresh = lambda scale=1.0: torch.randn(kw, cout, cin, generator=gen) * scale
    wp = wv = 0.0
    # chain A: no amsgrad, grad_averaging, weight decay, a roomy scratch: the first step (v = 0 selects ||g||^2), then the EMA
    S = PackState(shape, 50, lo=1, q=0)
    rp, rv, v = novo_step(L, S, fresh(), 0.0, None, 2048, 1e-3, 1, f'novograd {shape} step 1')
    wp, wv = max(wp, rp), max(wv, rv)
    rp, rv, v = novo_step(L, S, fresh(2.0), v, None, 2048, 1e-3, 1, f'novograd {shape} step 2 (EMA)')
    wp, wv = max(wp, rp), max(wv, rv)
    # chain B: amsgrad, no grad_averaging, no weight decay; scratch_floats = 2 forces one block (kept roomy for the 5.2 M
    # element tensor, whose one-block chain of 20 480 additions would leave the range the bound is derived for)
    sf = 1025 if huge else 2
    S = PackState(shape, 51, lo=0, q=0)
    rp, rv, v = novo_step(L, S, fresh(), 0.0, 0.0, sf, 0.0, 0, f'novograd {shape} amsgrad step 1')
    wp, wv = max(wp, rp), max(wv, rv)
    if not huge:
        rp, rv, v2 = novo_step(L, S, fresh(0.5), v, 10 * v, sf, 0.0, 0, f'novograd {shape} amsgrad, vmax above v')
        wp, wv = max(wp, rp), max(wv, rv)
        rp, rv, _ = novo_step(L, S, fresh(), v2, 0.01 * v2, sf, 0.0, 0, f'novograd {shape} amsgrad, vmax below v')
        wp, wv = max(wp, rp), max(wv, rv)
        rp, rv, _ = novo_step(L, S, fresh(), v2, None, 2, 1e-3, 0, f'novograd {shape} one block, wd without averaging')
        wp, wv = max(wp, rp), max(wv, rv)
    record('novograd', f'p/m {shape}', wp)
    record('novograd', f'v {shape}', wv)


# ================================================================================================================================
# w2l_pad_cast
# ================================================================================================================================

# the last: (3 + 4 * 4103) * 64 = 1 050 560 elements > 4096 blocks x 256 threads: the grid-stride loop takes a second round
PAD_CASES = [(3, 50, 29, 64, 13), (2, 333, 29, 64, 0), (1, 7, 64, 64, 28), (4, 4100, 29, 64, 3)]


@pytest.mark.parametrize('case', PAD_CASES, ids=lambda s: 'x'.join(map(str, s)))
def test_pad_cast(L, case):
    N, T, Cc, CP, halo = case
    assert case != PAD_CASES[-1] or (halo + N * (T + halo)) * CP > 4096 * 256
    gen = torch.Generator().manual_seed(60 + T)
    g0 = torch.randn(N, T, Cc, generator=gen)
    lay, cs, A = R.pad_cast_ref(g0.numpy(), N, T, Cc, CP, halo)
    rows = halo + N * (T + halo)
    g = Buf((N, T, Cc), init=g0)
    worst = 0.0
    for with_lo, with_cs in ((1, 1), (0, 1), (1, 0), (0, 0)):
        hi = Buf((rows, CP), torch.bfloat16)
        lo = Buf((rows, CP), torch.bfloat16) if with_lo else None
        col = Buf((CP,)) if with_cs else None
        L.check(L.lib.w2l_pad_cast(p(L, g), N, T, Cc, CP, halo, p(L, hi), p(L, lo), p(L, col), L.stream_ptr()))
        torch.cuda.synchronize()
        assert np.array_equal(hi.bits(), R.bf16_rne(lay.astype(np.float32))), 'hi must be bf16_rne of the shared-halo layout'
        zero = lay == 0
        assert zero[:halo].all() and zero[:, Cc:].all() and not hi.bits()[zero].any(), 'halo rows and pad columns are +0'
        if lo is not None:
            rec = hi.np().astype(np.float64) + lo.np()
            assert (np.abs(rec - lay) <= R.R_SPLIT * np.abs(lay)).all()
            assert np.array_equal(lo.bits(), R.split_bf16(lay.astype(np.float32))[1])
        if col is not None:
            r = ratio(col.np(), cs, R.dot_bound(A, N * T, cs))
            worst = max(worst, r)
            assert r <= 1, f'pad_cast {case}: colsum error / bound = {r}'
            assert not col.np()[Cc:].view(np.uint32).any()
        assert guards(g, hi, lo, col)
    record('pad_cast', f'colsum {case}', worst)
