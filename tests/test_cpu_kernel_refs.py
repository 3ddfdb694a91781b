"""The float64 references of tests/kernel_refs.py are themselves pinned here (no GPU): against torch's float64 conv1d and its
autograd, torch.optim.SGD in float64, the reference Novograd's recorded fixture and torch's own bf16 cast -- and each
family's error bound is shown to have teeth: a reference with one planted defect violates it."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import kernel_refs as R

GOLD = os.path.join(os.path.dirname(__file__), 'golden')


def bf(t):
    return t.to(torch.bfloat16).double()


def dw_inputs(N, Tout, C, K, s, d, extra=3, seed=0):
    g = torch.Generator().manual_seed(seed)
    rows = (Tout - 1) * s + (K - 1) * d + 1 + extra
    xp = bf(torch.randn(N, rows, C, generator=g))
    w = torch.randn(K, C, generator=g).double()
    dy = bf(torch.randn(N, Tout, C, generator=g))
    return xp, w, dy, rows


def rel(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


@pytest.mark.parametrize('shape', R.DW_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_dw_refs_match_conv1d_float64(shape):
    """dw_fwd_ref / dw_dgrad_ref / dw_wgrad_ref == F.conv1d(groups=C) and its autograd in float64, for every lens kind
    (the mask is applied to conv1d's output, which is what "rows t >= lens[n] are zero / count as zero" means)"""
    N, Tout, C, K, s, d = shape
    xp, w, dy, rows = dw_inputs(*shape)
    need = (Tout - 1) * s + (K - 1) * d + 1
    for kind in R.LENS_KINDS if N * Tout * C < (1 << 21) else ('ragged',):
        lens = R.dw_lens(kind, N, Tout)
        x = xp[:, :need].transpose(1, 2).contiguous().requires_grad_(True)          # [N, C, need]
        wt = w.t().reshape(C, 1, K).contiguous().requires_grad_(True)
        y = F.conv1d(x, wt, stride=s, dilation=d, groups=C)
        assert y.shape == (N, C, Tout)
        mask = torch.ones(N, 1, Tout, dtype=torch.float64)
        if lens is not None:
            mask = (torch.arange(Tout)[None, None, :] < torch.from_numpy(lens.astype(np.int64))[:, None, None]).double()
        ym = y * mask
        ym.backward(dy.transpose(1, 2))
        got, A = R.dw_fwd_ref(xp.numpy(), w.numpy(), N, Tout, C, K, s, d, lens)
        assert rel(got, ym.detach().transpose(1, 2).numpy()) <= 1e-12
        assert (A >= np.abs(got)).all()
        dwr, Aw, n_terms = R.dw_wgrad_ref(dy.numpy(), xp.numpy(), N, Tout, C, K, s, d, lens)
        assert rel(dwr, wt.grad.reshape(C, K).t().numpy()) <= 1e-12
        assert n_terms == int(mask.sum())
        if s == 1:
            Tp = need + 2                                                     # rows past the receptive field get nothing
            dx, Ad = R.dw_dgrad_ref(dy.numpy(), w.numpy(), N, Tp, Tout, C, K, d, lens)
            assert rel(dx[:, :need], x.grad.transpose(1, 2).numpy()) <= 1e-12
            assert not dx[:, need:].any()


SGD_CASES = [(R.SGD_MU, nest, wd) for nest, wd in sorted({(nest, wd) for _, nest, wd, *_ in R.SGD_FLAG_SETS})]
SGD_CASES += [(0.0, 0, 0.0), (0.0, 0, 1e-3)]          # no momentum buffer (torch rejects nesterov without momentum)


@pytest.mark.parametrize('clip', [None] + R.SGD_CLIPS)
@pytest.mark.parametrize('mu,nesterov,wd', SGD_CASES)
def test_sgd_ref_matches_torch_sgd_float64(mu, nesterov, wd, clip):
    """three steps (the first one creates the momentum buffer) of torch.optim.SGD on float64 tensors, with the clip written
    as torch's clip_grad_norm_ / clip_grad_value_ do it: grad.mul_(coef), grad.clamp_(-bound, bound); mu = 0 is the
    reference's m = None path"""
    g = torch.Generator().manual_seed(3)
    p0 = torch.randn(257, generator=g)
    p = torch.nn.Parameter(p0.double().clone())
    opt = torch.optim.SGD([p], lr=R.f32(R.SGD_LR), momentum=R.f32(mu), weight_decay=R.f32(wd), nesterov=bool(nesterov))
    pr, mr = p0.double().numpy(), None
    for step in range(3):
        gr = torch.randn(257, generator=g).double()
        p.grad = gr.clone()
        if clip is not None:
            p.grad.mul_(R.f32(clip[0])).clamp_(-R.f32(clip[1]), R.f32(clip[1]))
        opt.step()
        coef, bound = clip if clip is not None else (None, None)
        if mu == 0.0:
            P, M = R.sgd_ref(pr, gr.numpy(), None, 0, R.SGD_LR, mu, wd, nesterov, coef, bound)
            assert M is None
        else:
            P, M = R.sgd_ref(pr, gr.numpy(), np.full(257, np.nan) if step == 0 else mr, step == 0, R.SGD_LR, mu, wd, nesterov,
                             coef, bound)
            mr = M.v
            assert rel(mr, opt.state[p]['momentum_buffer'].numpy()) <= 1e-12
            assert (M.a >= np.abs(M.v)).all()
        pr = P.v
        assert rel(pr, p.detach().numpy()) <= 1e-12
        assert (P.a >= np.abs(P.v)).all() and np.isfinite(pr).all()


def test_sgd_ref_keeps_nan():
    g = np.array([1.0, np.nan, -2.0])
    for coef, bound in [(None, None)] + R.SGD_CLIPS:
        P, M = R.sgd_ref(np.ones(3), g, np.zeros(3), 0, 0.1, 0.9, 1e-3, 1, coef, bound)
        assert np.isnan(P.v).tolist() == [False, True, False] and np.isnan(M.v).tolist() == [False, True, False]


def test_novograd_ref_matches_reference_fixture():
    """4 steps against tests/golden/novograd_cases.npz (recorded from the reference's novograd.py), at the tolerance
    test_cpu_host.py::test_novograd_matches_reference_fixture uses for the same file"""
    z = np.load(os.path.join(GOLD, 'novograd_cases.npz'))
    for tag, kw in dict(plain=dict(lr=0.01, b1=0.95, b2=0.5, wd=1e-3, grad_averaging=True, ams=False),
                        ams=dict(lr=0.02, b1=0.9, b2=0.25, wd=0.0, grad_averaging=False, ams=True)).items():
        for i in (0, 1):
            p = z[f'{tag}/p0_{i}'].astype(np.float64)
            m, v = np.zeros_like(p), 0.0
            vmax = 0.0 if kw['ams'] else None
            for it in range(4):
                P, M, V, VM = R.novograd_ref(p, z[f'{tag}/grads{i}'][it], m, v, vmax, kw['lr'], kw['b1'], kw['b2'], 1e-8, kw['wd'],
                                             kw['grad_averaging'])
                p, m, v = P.v, M.v, float(V.v)
                if kw['ams']:
                    vmax = float(VM.v)
                    assert vmax >= v
            np.testing.assert_allclose(p, z[f'{tag}/p4_{i}'], rtol=1e-5, atol=1e-6)
            if i == 0:
                np.testing.assert_allclose(v, z[f'{tag}/v_0'], rtol=1e-5)


def test_novograd_depth_and_blocks():
    assert R.novograd_nblocks(64 * 64, 1025) == 1 and R.novograd_nblocks(128 * 64 * 11, 1025) == 22
    assert R.novograd_nblocks(128 * 64 * 11, 2) == 1 and R.novograd_nblocks(1024 * 1024 * 5, 4096) == 1024
    assert R.novograd_norm_depth(1024 * 1024 * 5, 1024) == 1 + 20 + 8 + 4 + 8
    assert R.novograd_norm_depth(128 * 64 * 11, 1) == 1 + 352 + 8 + 1 + 8


def test_bf16_rne_is_torch_bfloat16():
    g = torch.Generator().manual_seed(11)
    x = torch.cat([torch.randn(520_000, generator=g) * torch.exp(8 * torch.randn(520_000, generator=g)),
                   torch.randint(-2 ** 31, 2 ** 31 - 1, (520_000,), generator=g, dtype=torch.int64).to(torch.int32).view(torch.float32)])
    x = x[~torch.isnan(x)]
    assert x.numel() >= 1_000_000
    want = x.to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(R.bf16_rne(x.numpy()), want)
    # ties: exactly half an ulp above an even / an odd bf16 value; just below and just above the tie; the carry into the exponent
    bits = np.array([0x3F808000, 0x3F818000, 0x3F807FFF, 0x3F808001, 0x3FFF8000, 0x7F7F8000, 0xBF808000, 0x00008000, 0x00018000],
                    dtype=np.uint32)
    want = np.array([0x3F80, 0x3F82, 0x3F80, 0x3F81, 0x4000, 0x7F80, 0xBF80, 0x0000, 0x0002], dtype=np.uint16)
    assert np.array_equal(R.bf16_rne(bits.view(np.float32)), want)
    assert np.array_equal(torch.from_numpy(bits.view(np.float32).copy()).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16), want)
    assert np.isnan(R.bf16_to_f32(R.bf16_rne(np.array([np.nan], dtype=np.float32)))).all()
    hi, lo = R.split_bf16(x.numpy()[:100_000])
    xs = x.numpy()[:100_000].astype(np.float64)
    ok = np.isfinite(xs) & (np.abs(xs) > 1e-30) & (np.abs(xs) < 1e38)
    rec = R.bf16_to_f32(hi).astype(np.float64) + R.bf16_to_f32(lo).astype(np.float64)
    assert (np.abs(rec - xs)[ok] <= R.R_SPLIT * np.abs(xs)[ok]).all()


# ---- the bounds have teeth: one planted defect each must violate them ---------------------------------------------------------

def violates(defect, clean, bound):
    return bool((np.abs(defect - clean) > bound).any())


TAIL = R.DW_SHAPES[1]                 # 3 x 301 rows = 903 = 3 x 256 + a 135-row tail


def test_bound_catches_depthwise_defects():
    N, Tout, C, K, s, d = TAIL
    xp, w, dy, rows = dw_inputs(*TAIL)
    xp, w, dy = xp.numpy(), w.numpy(), dy.numpy()
    lens = R.dw_lens('ragged', N, Tout)
    for r_out in (R.R_BF16, R.R_SPLIT):
        y, A = R.dw_fwd_ref(xp, w, N, Tout, C, K, s, d, lens)
        b = R.dot_bound(A, K, y, r_out)
        assert not violates(y, y, b)
        # the last tap dropped
        wz = w.copy()
        wz[K - 1] = 0
        assert violates(R.dw_fwd_ref(xp, wz, N, Tout, C, K, s, d, lens)[0], y, b)
        # lens off by one, either way
        assert violates(R.dw_fwd_ref(xp, w, N, Tout, C, K, s, d, lens + 1)[0], y, b)
        assert violates(R.dw_fwd_ref(xp, w, N, Tout, C, K, s, d, np.maximum(lens - 1, 0))[0], y, b)
        # utterance n's window starts at n*Tout instead of n*x_rows
        flat = xp.reshape(N * rows, C)
        bad = np.stack([flat[n * Tout: n * Tout + rows] for n in range(N)])
        assert violates(R.dw_fwd_ref(bad, w, N, Tout, C, K, s, d, lens)[0], y, b)
    # one row of the 256-row tail skipped in the weight gradient (fp32 output), with the sentinel rows out of reach
    dw, Aw, nt = R.dw_wgrad_ref(dy, xp, N, Tout, C, K, s, d, None)
    assert nt == 903
    bw = R.dot_bound(Aw, nt, dw)
    dz = dy.copy().reshape(N * Tout, C)
    dz[3 * 256 + 77] = 0
    assert violates(R.dw_wgrad_ref(dz.reshape(N, Tout, C), xp, N, Tout, C, K, s, d, None)[0], dw, bw)
    # and in the data gradient (bf16 output): the last tap dropped, lens off by one
    Tp = rows
    dx, Ad = R.dw_dgrad_ref(dy, w, N, Tp, Tout, C, K, d, lens)
    bd = R.dot_bound(Ad, K, dx, R.R_BF16)
    assert violates(R.dw_dgrad_ref(dy, wz, N, Tp, Tout, C, K, d, lens)[0], dx, bd)
    assert violates(R.dw_dgrad_ref(dy, w, N, Tp, Tout, C, K, d, lens + 1)[0], dx, bd)


def test_bound_catches_nesterov_with_old_momentum():
    g = torch.Generator().manual_seed(5)
    p, gr, m = (torch.randn(4096, generator=g).numpy().astype(np.float64) for _ in range(3))
    P, M = R.sgd_ref(p, gr, m, 0, R.SGD_LR, R.SGD_MU, 1e-3, 1)
    lr, mu, wd = R.f32(R.SGD_LR), R.f32(R.SGD_MU), R.f32(1e-3)
    g1 = gr + wd * p
    bad = p - lr * (g1 + mu * m)                    # the look-ahead taken with the momentum of the step before
    assert violates(bad, P.v, P.bound())
    assert not violates(p - lr * (g1 + mu * (mu * m + g1)), P.v, P.bound())


def test_bound_catches_nonzero_halo_row():
    g = torch.Generator().manual_seed(6)
    N, T, C, CP, halo = 3, 50, 29, 64, 13
    x = torch.randn(N, T, C, generator=g).numpy()
    lay, cs, A = R.pad_cast_ref(x, N, T, C, CP, halo)
    assert lay.shape == (halo + N * (T + halo), CP) and not lay[:halo].any() and not lay[:, C:].any()
    assert np.array_equal(lay[halo + (T + halo) + 7, :C], x[1, 7].astype(np.float64))
    b = R.R_SPLIT * np.abs(lay)
    bad = lay.copy()
    bad[0, 0] = 2.0 ** -126
    assert violates(bad, lay, b) and not violates(lay, lay, b)
    # a column sum that misses one row
    assert violates(cs - np.concatenate([x[2, 49], np.zeros(CP - C)]), cs, R.dot_bound(A, N * T, cs))
