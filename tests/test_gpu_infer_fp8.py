"""The fused fp8 inference path on a real MI355X: the e4m3 convolution with the whole-unit epilogue
(w2l_conv1d_igemm_bnact_fp8) through the C ABI against the chain it replaces (w2l_conv1d_igemm_fp8 into a bf16 y, then
w2l_bn_act_fwd_q) and an fp64 evaluation of the dequantised operands; ``model.infer`` of ``precision='fp8'`` models against
the fp8 evaluation-mode forward with the fp32 ``infer`` of the same weights as the truth."""
import ctypes as C
import os
import warnings

import numpy as np
import pytest
import torch

from gpu_helpers import build_jasper, build_w2l
from test_gpu_infer import CONV_SHAPES, _bf16, _f64, _fixture_model, _ref_rows

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the shapes of the tables the e4m3 kernel admits: stride 1, Cin a multiple of 128
F8_SHAPES = [s for s in CONV_SHAPES if s[3] == 1 and s[0] % 128 == 0]
assert len(F8_SHAPES) >= 15 and (256, 256, 11, 1, 1) in F8_SHAPES and (896, 896, 29, 1, 2) in F8_SHAPES


def _e4m3_table():
    """byte -> value of OCP e4m3 (e4m3fn: bias 7, no infinities, S.1111.111 = NaN)"""
    t = np.zeros(256)
    for b in range(256):
        sgn, e, m = -1.0 if b & 0x80 else 1.0, (b >> 3) & 0xF, b & 7
        if e == 15 and m == 7:
            t[b] = np.nan
        elif e == 0:
            t[b] = sgn * (m / 8.0) * 2.0 ** -6
        else:
            t[b] = sgn * (1 + m / 8.0) * 2.0 ** (e - 7)
    return t


E4M3 = _e4m3_table()


def _deq(q, scale):
    return E4M3[q.cpu().numpy()] / scale


def _quant(t_bf16, scale):
    from wav2letter_pytorch_amd._lib import check, lib, ptr, stream_ptr
    q = torch.empty(t_bf16.shape, dtype=torch.uint8, device=t_bf16.device)
    check(lib.w2l_quantize_e4m3(ptr(t_bf16), 0, t_bf16.numel(), scale, ptr(q), stream_ptr()), 'w2l_quantize_e4m3')
    return q


def _pow2(amax):
    return 2.0 ** np.floor(np.log2(448.0 / amax))


class _Problem:
    """one convolution on e4m3 operands with everything the epilogue may take, and its fp64 accumulators"""

    def __init__(self, shape, N, Tout, seed):
        from wav2letter_pytorch_amd._lib import check, lib, ptr, stream_ptr
        cin, cout, k, s, d = shape
        g = torch.Generator().manual_seed(seed)
        dev = torch.device('cuda')
        self.shape, self.N, self.Tout = shape, N, Tout
        self.Tin = Tin = (Tout - 1) * s + (k - 1) * d + 1
        x = _bf16(torch.randn(N, Tin, cin, generator=g)).to(dev)
        w = _bf16(torch.randn(k, cout, cin, generator=g) / np.sqrt(cin * k)).to(dev)
        self.ws = float(_pow2(float(w.abs().max())))
        self.wq = _quant(w, self.ws)
        self.xq = {16.0: _quant(x, 16.0)}                             # (randn inputs: 16 |x| stays far below 448)
        self.bias = (0.1 * torch.randn(cout, generator=g)).to(dev)
        gamma, beta = (1 + 0.2 * torch.randn(cout, generator=g)).to(dev), (0.3 * torch.randn(cout, generator=g)).to(dev)
        rmean, rvar = (0.2 * torch.randn(cout, generator=g)).to(dev), (0.5 + torch.rand(cout, generator=g)).to(dev)
        self.res = _bf16(torch.randn(N, Tout, cout, generator=g)).to(dev)
        self.lens = torch.randint(Tout // 2, Tout + 1, (N,), generator=g, dtype=torch.int32)
        self.lens[0] = Tout
        self.lens_d = self.lens.to(dev)
        self.scale, self.shift = torch.empty(cout, device=dev), torch.empty(cout, device=dev)
        check(lib.w2l_bn_finalize(None, 0, cout, 1, ptr(gamma), ptr(beta), 1e-3, 0.1, ptr(rmean), ptr(rvar), None, None,
                                  ptr(self.scale), ptr(self.shift), stream_ptr()), 'bn_finalize')
        self.ones, self.zeros = torch.ones(cout, device=dev), torch.zeros(cout, device=dev)
        self.acc = {}
        wf = _deq(self.wq, self.ws)
        for sc, xq in self.xq.items():
            xf = _deq(xq, sc)
            a = np.zeros((N, Tout, cout))
            for kk in range(k):
                a += xf[:, kk * d: kk * d + (Tout - 1) * s + 1: s, :] @ wf[kk].T
            self.acc[sc] = a

    def reference(self, x_scale, with_bias, act, masked, with_res):
        z = (self.acc[x_scale] + (_f64(self.bias) if with_bias else 0.0)) * _f64(self.scale) + _f64(self.shift)
        if with_res:
            z = z + _f64(self.res)
        z = np.clip(z, 0, 20) if act == 1 else (np.maximum(z, 0) if act == 2 else z)
        if masked:
            z = z * (np.arange(self.Tout)[None, :, None] < self.lens.numpy()[:, None, None])
        return z

    def fused(self, x_scale, with_bias, act, masked, with_res, pl, pr, reflect, R, q_scale, want_hi=True, want_q=True, clip=None):
        from wav2letter_pytorch_amd._lib import BnActEpi, check, lib, ptr, stream_ptr
        cin, cout, k, s, d = self.shape
        N, Tout, dev = self.N, self.Tout, self.wq.device
        out = torch.full((N, R, cout), 7.0, dtype=torch.bfloat16, device=dev) if want_hi else None
        outq = torch.full((N, R, cout), 0x77, dtype=torch.uint8, device=dev) if want_q else None
        e = BnActEpi()
        e.scale, e.shift, e.res = ptr(self.scale), ptr(self.shift), (ptr(self.res) if with_res else None)
        e.act, e.lens, e.out_hi, e.out_rows = act, (ptr(self.lens_d) if masked else None), ptr(out), R
        e.pad_l, e.pad_r, e.pad_mode = pl, pr, int(reflect)
        check(lib.w2l_conv1d_igemm_bnact_fp8(ptr(self.xq[x_scale]), self.Tin * cin, N * self.Tin, ptr(self.wq),
                                             1.0 / (x_scale * self.ws), ptr(self.bias) if with_bias else None, C.byref(e),
                                             ptr(outq), q_scale, ptr(clip), N, cin, cout, Tout, k, d, stream_ptr()),
              'w2l_conv1d_igemm_bnact_fp8')
        torch.cuda.synchronize()
        return out, outq

    def chain(self, x_scale, with_bias, act, masked, with_res, pl, pr, reflect, R, q_scale, clip=None):
        """the launches the fp8 evaluation-mode forward makes for this unit"""
        from wav2letter_pytorch_amd._lib import BnActDesc, check, lib, ptr, stream_ptr
        cin, cout, k, s, d = self.shape
        N, Tout, dev = self.N, self.Tout, self.wq.device
        rows = pl + Tout + pr
        y = torch.empty(N, Tout, cout, dtype=torch.bfloat16, device=dev)
        check(lib.w2l_conv1d_igemm_fp8(ptr(self.xq[x_scale]), self.Tin * cin, N * self.Tin, ptr(self.wq), ptr(y), 0,
                                       1.0 / (x_scale * self.ws), None, ptr(self.bias) if with_bias else None, None, N, cin, cout,
                                       Tout, k, d, stream_ptr()), 'w2l_conv1d_igemm_fp8')
        dsc = BnActDesc()
        dsc.N, dsc.T, dsc.C, dsc.y, dsc.y_f32 = N, Tout, cout, y.data_ptr(), 0
        dsc.scale, dsc.shift = self.scale.data_ptr(), self.shift.data_ptr()
        if with_res:
            dsc.y2, dsc.scale2, dsc.shift2 = self.res.data_ptr(), self.ones.data_ptr(), self.zeros.data_ptr()
        dsc.act, dsc.drop_p = act, 0.0
        dsc.lens = self.lens_d.data_ptr() if masked else None
        if clip is not None:
            dsc.q_clipped = clip.data_ptr()
        o = torch.empty(N, rows, cout, dtype=torch.bfloat16, device=dev)
        oq = torch.empty(N, rows, cout, dtype=torch.uint8, device=dev)
        check(lib.w2l_bn_act_fwd_q(C.byref(dsc), ptr(o), None, ptr(oq), q_scale, rows, pl, pr, int(reflect), stream_ptr()),
              'w2l_bn_act_fwd_q')
        torch.cuda.synchronize()
        return o, oq


def _cases(k, d):
    pad = (k - 1) * d
    # name, bias + reflect halo, act, masked, residual operand, pads, scale of the e4m3 output (FP8_ACT_SCALE of the act)
    cases = [('w2l', True, 1, False, False, (pad // 2, pad - pad // 2), 16.0),
             ('jasper', False, 2, True, False, (max(pad // 2, 1), max(pad // 2, 1)), 8.0),
             ('jasper+res', False, 2, True, True, (28, 28), 8.0)]
    if k == 1:        # as infer() launches a residual branch: affine only, dense output (no halo, no mask, exactly Tout rows)
        cases.append(('residual branch', False, 0, False, False, (0, 0), 8.0))
    return cases


@pytest.mark.parametrize('N', [1, 3, 32])
@pytest.mark.parametrize('shape', F8_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_fused_fp8_kernel_against_chain_and_fp64(shape, N):
    """Per shape the Wav2Letter case (bias, reflect halo, clamp, scale 16), the Jasper cases (zero halo, ReLU, ragged lengths,
    with and without the residual operand, scale 8) and, for 1x1, the dense residual-branch case.  Operands are e4m3 bytes made
    by w2l_quantize_e4m3; the reference is the fp64 evaluation of the dequantised operands through the same epilogue.  RMS
    error of the fused bf16 output <= that of the chain's, RMS error of the dequantised fused e4m3 output <= that of the
    chain's e4m3 copy (both bounds measured here, against existing code)."""
    cin, cout, k, s, d = shape
    Tout = 150 if N < 32 else 70
    P = _Problem(shape, N, Tout, seed=cin * 31 + cout * 7 + k + N)
    for name, reflect, act, masked, with_res, (pl, pr), q_scale in _cases(k, d):
        x_scale = 16.0
        ref_t = P.reference(x_scale, reflect, act, masked, with_res)
        rows = _ref_rows(Tout, pl, pr, reflect)
        ref = np.where(rows[None, :, None] >= 0, ref_t[:, np.maximum(rows, 0), :], 0.0)
        ext = pl + Tout + pr
        R = ext + (3 if name != 'residual branch' else 0)
        args = (x_scale, reflect, act, masked, with_res, pl, pr, reflect, R, q_scale)
        f_hi, f_q = P.fused(*args)
        c_hi, c_q = P.chain(*args)
        assert bool((f_hi[:, ext:] == 7.0).all()) and bool((f_q[:, ext:] == 0x77).all()), (name, 'rows beyond the extent written')
        only_q = P.fused(*args, want_hi=False)[1]
        assert torch.equal(only_q, f_q), (name, 'the e4m3-only form differs from the two-output form')
        only_hi = P.fused(*args, want_q=False)[0]
        assert torch.equal(only_hi.view(torch.int16), f_hi.view(torch.int16)), (name, 'the bf16-only form differs')

        def rms(v):
            return float(np.sqrt(np.mean((v - ref) ** 2)))
        r_hi = {'fused': rms(_f64(f_hi[:, :ext])), 'chain': rms(_f64(c_hi))}
        r_q = {'fused': rms(_deq(f_q[:, :ext], q_scale)), 'chain': rms(_deq(c_q, q_scale))}
        print(f'[bnact fp8] {shape} N={N} {name}: bf16 rms fused {r_hi["fused"]:.3e} chain {r_hi["chain"]:.3e}; '
              f'e4m3 rms fused {r_q["fused"]:.3e} chain {r_q["chain"]:.3e}')
        assert r_hi['fused'] <= r_hi['chain'], (name, r_hi)
        assert r_q['fused'] <= r_q['chain'], (name, r_q)
        # halo rows: byte-equal to the interior rows they mirror (reflect) or zero, in both outputs
        f16 = f_hi.view(torch.int16)
        for r, t in enumerate(rows):
            if r - pl == t:
                continue
            if t >= 0:
                assert torch.equal(f_q[:, r], f_q[:, pl + t]) and torch.equal(f16[:, r], f16[:, pl + t]), (name, r, t)
            else:
                assert bool((f_q[:, r] == 0).all()) and bool((f16[:, r] == 0).all()), (name, r)
        if masked:
            for n in range(N):
                ln = int(P.lens[n])
                assert bool((f_q[n, pl + ln: pl + Tout] == 0).all()) and bool((f16[n, pl + ln: pl + Tout] == 0).all()), (name, n)


@pytest.mark.parametrize('N', [1, 3])
def test_fused_fp8_saturation_counter(N):
    """ReLU output at scale 8 saturates beyond 448 / 8 = 56.  A residual operand of 100 on 37 chosen elements puts exactly
    those (less the ones the length mask zeroes) beyond 56 and leaves every other element below 20: nothing is near the
    threshold, and the counter must equal the count over the fp64 reference; the chain's counter agrees."""
    shape = (256, 256, 11, 1, 1)
    Tout = 150
    P = _Problem(shape, N, Tout, seed=99 + N)
    g = torch.Generator().manual_seed(5)
    idx = torch.randperm(N * Tout * 256, generator=g)[:37]
    flat = P.res.view(-1)
    flat[idx.cuda()] = 100.0
    ref = P.reference(16.0, False, 2, True, True)
    want = int((np.abs(ref) > 56.0).sum())
    assert not ((np.abs(ref) > 40.0) & (np.abs(ref) < 72.0)).any() and 0 < want <= 37
    clip = torch.zeros(1, dtype=torch.int64, device='cuda')
    clip2 = torch.zeros(1, dtype=torch.int64, device='cuda')
    args = (16.0, False, 2, True, True, 5, 5, False, 160, 8.0)
    _, f_q = P.fused(*args, clip=clip)
    P.chain(*args, clip=clip2)
    print(f'[bnact fp8] saturation: fp64 {want}, fused {int(clip.item())}, chain {int(clip2.item())}')
    assert int(clip.item()) == want and int(clip2.item()) == want
    assert int((f_q[:, 5:5 + Tout] == 0x7E).sum()) == want            # 0x7E = +448: the saturated elements, and only they
    P.fused(*args, want_hi=False, clip=clip)
    assert int(clip.item()) == 2 * want                              # the counter accumulates; the e4m3-only form counts too


def test_fused_fp8_rejects_what_the_kernel_rejects():
    from wav2letter_pytorch_amd._lib import BnActEpi, lib, ptr, stream_ptr
    dev = torch.device('cuda')
    buf = torch.zeros(1 << 20, dtype=torch.uint8, device=dev)
    e = BnActEpi()
    e.out_hi, e.out_rows, e.pad_l, e.pad_r = ptr(buf), 64, 0, 0

    def call(cin=128, cout=64, pl=0, rows=64, out_q=buf):
        e.pad_l, e.out_rows = pl, rows
        return lib.w2l_conv1d_igemm_bnact_fp8(ptr(buf), 64 * cin, 64, ptr(buf), 1.0, None, C.byref(e), ptr(out_q), 8.0, None, 1,
                                              cin, cout, 64, 1, 1, stream_ptr())
    assert call(cin=64) != 0 and call(cout=32) != 0 and call(pl=97, rows=64 + 97) != 0
    assert call() == 0
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------- models
def _count_launches(fn):
    """library entry points that enqueue kernels, called by one run of fn (tools/bench_infer.py count_launches)"""
    from wav2letter_pytorch_amd import _lib
    names = list(_lib.TRACE_NAMES)
    saved = {n: getattr(_lib.lib, n) for n in names if hasattr(_lib.lib, n)}
    counts = {}

    def wrap(n, f):
        def inner(*a):
            counts[n] = counts.get(n, 0) + 1
            return f(*a)
        return inner
    for n, f in saved.items():
        setattr(_lib.lib, n, wrap(n, f))
    try:
        fn()
    finally:
        for n, f in saved.items():
            setattr(_lib.lib, n, f)
    return sum(counts.values()), counts


def _boundaries(eng, cp0):
    """units of an fp8 engine that run on bf16 operands and whose output carries an e4m3 copy (one quantise launch each), and
    the units whose main convolution runs on e4m3 operands"""
    from wav2letter_pytorch_amd.engine import infer_copies
    copies = infer_copies(eng.units, True, True, cp0)
    e4m3, bound = [], []
    for ui, u in enumerate(eng.units):
        src_q = copies[u.src][1]
        on_q = src_q and u.dw is None and u.main.stride == 1
        if on_q:
            e4m3.append(ui)
        elif copies[ui + 1][1]:
            bound.append(ui)
    return e4m3, bound


def _rms(a, b, valid):
    d = (a.double() - b.double())[valid]
    return float(d.pow(2).mean().sqrt())


def _ab(name, make, x, il, record):
    """fused fp8 infer, fp8 evaluation-mode forward, fp32 infer (the truth) of one network"""
    from wav2letter_pytorch_amd.decoder import argmax_indices
    m8, m32, mb = make('fp8'), make('fp32'), make('bf16')
    xd = x.cuda()
    with warnings.catch_warnings():
        warnings.simplefilter('error')                     # no warning: the fp8 engine no longer falls back
        fused, fl = m8.infer(xd, il)
    eng = m8.engine()
    assert eng.fp8_saturated() == 0
    with torch.no_grad():
        plain, pll = m8(xd, il)
    assert eng.fp8_saturated() == 0
    truth, tl = m32.infer(xd, il)
    np.testing.assert_array_equal(np.asarray(fl), np.asarray(pll))
    np.testing.assert_array_equal(np.asarray(fl), np.asarray(tl))
    T = truth.shape[1]
    lens = torch.as_tensor(np.asarray(fl)).long() if fl is not None else torch.full((truth.shape[0],), T)
    valid = (torch.arange(T)[None, :] < lens[:, None]).cuda()
    if float(truth.max()) > 0:                              # Jasper's evaluation output is a softmax: compare in the log domain
        fused, plain, truth = (t.clamp_min(1e-30).log() for t in (fused, plain, truth))
    r_f, r_p = _rms(fused, truth, valid), _rms(plain, truth, valid)
    am = argmax_indices(truth)
    ag_f = float((argmax_indices(fused) == am)[valid].float().mean())
    ag_p = float((argmax_indices(plain) == am)[valid].float().mean())
    # launch budget: the bf16 infer's launches plus one quantise launch per bf16-to-e4m3 boundary unit
    mb.infer(xd, il)                                       # (a first call also packs weights, folds BatchNorm and measures)
    n8 = _count_launches(lambda: m8.infer(xd, il))[0]
    nb = _count_launches(lambda: mb.infer(xd, il))[0]
    e4m3, bound = _boundaries(eng, 64)
    line = (f'{name}: rms vs fp32 infer: fused fp8 {r_f:.4e}, fp8 eval forward {r_p:.4e} (ratio {r_f / max(r_p, 1e-30):.3f}); '
            f'argmax agreement with fp32: fused {ag_f:.4f}, eval forward {ag_p:.4f}; launches fp8 infer {n8}, bf16 infer {nb}, '
            f'boundary units {bound}; units on e4m3 operands {e4m3}')
    print('[infer fp8] ' + line)
    record.append(line)
    assert n8 == nb + len(bound), (n8, nb, bound)
    assert r_f <= 1.10 * r_p, (r_f, r_p)
    return e4m3, bound


def _record(lines):
    """the model-level figures, kept beside the timing of tools/bench_infer.py --precision fp8 (which rewrites its own part)"""
    path = os.path.join(ROOT, 'profiles', 'infer_fp8_ab.txt')
    try:
        old = open(path).read().split('\n') if os.path.exists(path) else []
        keep = [l for l in old if not any(l.startswith('[test] ' + n.split(':')[0] + ':') for n in lines)]
        with open(path, 'w') as f:
            f.write('\n'.join([l for l in keep if l] + ['[test] ' + l for l in lines]) + '\n')
    except OSError:
        pass


@pytest.mark.parametrize('case', ['w2l_ml1', 'w2l_ml3', 'w2l_mix5', 'jasper_dense'])
def test_infer_fp8_fixtures(case):
    """The fixtures are narrow: w2l_* have no 128-multiple widths in front of a stride-1 convolution unless stated by the
    printed line (units on e4m3 operands), so they mostly exercise the boundary rules and the bf16 launches of an fp8 engine."""
    z = _fixture_model(case)[1]
    x, il = torch.from_numpy(z['x']), torch.from_numpy(z['in_lens'])
    rec = []
    _ab(case, lambda p: _fixture_model(case, p)[0], x, il, rec)
    _record(rec)


@pytest.mark.parametrize('net', ['wav2letter', 'jasper10x5'])
def test_infer_fp8_full_size(net):
    """The full 21-layer Wav2Letter at N=32 x T=1000 and Jasper 10x5 at N=16, random weights as
    test_infer_full_size_bf16_against_fp32_oracle builds them: rms(fused - truth) <= 1.10 rms(unfused - truth) over valid
    frames -- both are realisations of the same quantisation noise over 10^5..10^7 elements."""
    from oracle import w2l_oracle as O
    if net == 'wav2letter':
        layers = [l[:4] + (0.0,) for l in O.W2L_LAYERS]
        sd = O.init_wav2letter_state(layers, seed=0)

        def make(p):
            return build_w2l(layers, sd, p).eval()
        n = 32
    else:
        from wav2letter_pytorch_amd import Jasper
        from wav2letter_pytorch_amd.defaults import jasper10x5_model
        cfg = jasper10x5_model()
        blocks = [dict(b) for b in cfg.jasper_blocks]
        torch.manual_seed(7)
        sd = {k: v.detach().clone() for k, v in Jasper(cfg).state_dict().items()}

        def make(p):
            return build_jasper(blocks, sd, p).eval()
        n = 16
    x, il, _, _ = O.synthetic_batch(n, 1000, seed=1234)
    rec = []
    e4m3, bound = _ab(f'{net} N={n} T=1000', make, x, il, rec)
    _record(rec)
    assert len(e4m3) >= 10, e4m3                       # the wide units do run on e4m3 operands
    if net == 'wav2letter':
        assert bound == [0], bound                     # the stride-2 first convolution: the one bf16-to-e4m3 boundary


# ------------------------------------------------------------------------------------------------------ nothing else moved
@pytest.mark.parametrize('case', ['w2l_mix5', 'jasper_dense'])
@pytest.mark.parametrize('precision', ['bf16', 'fp32'])
def test_bf16_and_fp32_infer_unchanged_by_the_fp8_plan(case, precision, monkeypatch):
    """bf16 / fp32 engines never take an e4m3 copy: infer() with the buffer plan as it is equals, bit for bit, infer() with
    the second output disabled outright (every activation bf16 only)."""
    from wav2letter_pytorch_amd import engine as E
    model, z = _fixture_model(case, precision)
    x, il = torch.from_numpy(z['x']).cuda(), torch.from_numpy(z['in_lens'])
    out, _ = model.infer(x, il)
    assert all(c == (True, False) for c in E.infer_copies(model.engine().units, True, False, 64))
    monkeypatch.setattr(E, 'infer_copies', lambda units, head, fp8, cp0: [(True, False)] * (len(units) + 1))
    model2, _ = _fixture_model(case, precision)
    out2, _ = model2.infer(x, il)
    assert torch.equal(out, out2)


def test_fp8_training_step_between_two_infers_keeps_the_operands_current():
    """infer, one fp8 training step (fused SGD keeps the e4m3 weight operands current), infer again: the second infer sees
    the updated weights -- it equals the infer of a fresh model loaded from the state dict."""
    from oracle import w2l_oracle as O
    layers = [(256, 11, 2, 1, 0.0), (256, 11, 1, 1, 0.0), (384, 13, 1, 1, 0.0)]
    sd = O.init_wav2letter_state(layers, seed=3)
    model = build_w2l(layers, sd, 'fp8')
    x, il, tg, tl = O.synthetic_batch(4, 200, seed=11, s_lo=5, s_hi=15)
    xd = x.cuda()
    model.eval()
    first, _ = model.infer(xd, il)
    first = first.clone()
    model.train()
    from wav2letter_pytorch_amd.optim import FusedSGD
    opt = FusedSGD.from_sgd(torch.optim.SGD(model.parameters(), lr=0.05, momentum=0.9, nesterov=True, weight_decay=1e-4))
    opt.zero_grad(set_to_none=True)
    out, out_lens = model(xd, il)
    loss = model.criterion(out.transpose(0, 1), tg, out_lens, tl)
    loss.backward()
    opt.step()
    opt.join()
    model.eval()
    second, _ = model.infer(xd, il)
    fresh = build_w2l(layers, {k: v.detach().clone() for k, v in model.state_dict().items()}, 'fp8').eval()
    want, _ = fresh.infer(xd, il)
    assert not torch.equal(first, second)
    scales = [[u.main.weight._w2l_fp8['scale'] for u in m.engine().units if '_w2l_fp8' in u.main.weight.__dict__]
              for m in (model, fresh)]
    assert scales[0] and len(scales[0]) == len(scales[1])
    if scales[0] == scales[1]:
        assert torch.equal(second, want)
    else:       # (a weight's amax crossed a power of two: the trained model adopts the new scale FP8_RESCALE_LAG versions later)
        assert float((second - want).abs().max()) < 0.1 * float((first - want).abs().max())
