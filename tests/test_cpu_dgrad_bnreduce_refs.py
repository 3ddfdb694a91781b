"""The float64 reference of the data gradient fused with the BatchNorm-backward reduce (bn_refs.dgrad_bnreduce_ref, used by
tests/test_gpu_dgrad_bnreduce_direct.py) pinned on the CPU: against torch float64 autograd of
conv1d(pad(dropout_mask * act(batch_norm(y)))) contracted with dy, against the same sums formed row by row (the fold is linear),
and the planted defects shown to exceed the bound of every GPU case they can show on -- and to change nothing where they cannot."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bn_refs as B
from bn_refs import Case, DgCase
from direct_helpers import ratio

EPS = 1e-3

# reflect and zero padding, act 0 / 1 / 2, p = 0 and p > 0, ragged lens, pad_r == T - 1, a unit without BatchNorm, Tout != T
TORCH_CASES = [
    DgCase(Case('t_clamp_drop_ragged', 3, 11, 8, act=1, p=0.3, lens='ragged', pad_l=4, pad_r=4, pad_mode=1, seed=81), 5, 5, 2, 10),
    DgCase(Case('t_relu_zero', 2, 9, 16, act=2, pad_l=2, pad_r=1, pad_mode=0, seed=82), 3, 3, 1, 2),
    DgCase(Case('t_none_drop_longest_mirror', 3, 7, 8, act=0, p=0.5, lens='over', pad_l=0, pad_r=6, pad_mode=1, seed=83), 4, 4, 2, 7),
    DgCase(Case('t_nobn_ragged', 3, 10, 8, bn1=0, act=1, lens='ragged', pad_l=3, pad_r=3, pad_mode=1, seed=84), 6, 7, 1, 9),
    DgCase(Case('t_relu_zero_drop_ragged', 3, 10, 8, act=2, p=0.25, lens='ragged', pad_l=3, pad_r=3, pad_mode=0, seed=85), 6, 7, 1, 6),
]


def rel(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def torch_model(g, D):
    """the unit and its consumer in torch float64, BatchNorm in train mode on the case's y; returns the gradient wrt the padded
    activation [N][Tp][C], d beta / d gamma (or the summed gradient wrt y without BatchNorm) and the float64 statistics"""
    c = g.u
    N, T, Cc = c.N, c.T, c.C
    rng = np.random.default_rng(9)
    t64 = lambda v: torch.from_numpy(np.asarray(v, dtype=np.float64))
    x = t64(D['y']).transpose(1, 2).contiguous().requires_grad_(True)                # [N][C][T]
    st, ga, be, z = {}, None, None, x
    if c.bn1:
        ga, be = t64(rng.random(Cc) + 0.5).requires_grad_(True), t64(rng.standard_normal(Cc)).requires_grad_(True)
        y64 = D['y'].astype(np.float64)
        mean, inv = y64.mean((0, 1)), 1 / np.sqrt(y64.var((0, 1)) + EPS)
        st = dict(mean=mean, invstd=inv, scale=ga.detach().numpy() * inv, shift=be.detach().numpy() - mean * ga.detach().numpy() * inv)
        z = F.batch_norm(x, None, None, ga, be, training=True, eps=EPS)
    if c.p > 0:
        z = z * torch.from_numpy(B.unpack_keep(D['mask'], N, T, Cc)).transpose(1, 2).double() * B.inv_keep_f32(c.p)
    a = z.clamp(0, 20) if c.act == 1 else (F.relu(z) if c.act == 2 else z)
    if D['lens'] is not None:
        a = a.masked_fill(torch.arange(T)[None, None, :] >= torch.from_numpy(D['lens'].astype(np.int64))[:, None, None], 0.0)
    ap = F.pad(a, (c.pad_l, c.pad_r), mode='reflect' if c.pad_mode == 1 else 'constant')
    ap.retain_grad()
    out = F.conv1d(ap, t64(D['w']), dilation=g.dil)                                  # [N][Cout][Tout]
    assert out.shape[2] == g.Tout
    frames = D['dy'][g.halo:].reshape(N, g.per, g.Cout)[:, :g.Tout]
    (out * t64(frames).transpose(1, 2)).sum().backward()
    return dict(dxp=ap.grad.transpose(1, 2).numpy(), st=st, dbeta=be.grad.numpy() if c.bn1 else x.grad.sum((0, 2)).numpy(),
                dgamma=ga.grad.numpy() if c.bn1 else None)


@pytest.mark.parametrize('g', TORCH_CASES, ids=lambda g: g.name)
def test_ref_matches_torch_float64(g):
    c = g.u
    D = dict(B.make_dg_case(g, zero_halo=True))
    tm = torch_model(g, D)
    D.update(tm['st'])                                  # float64 statistics, as torch has them
    ref = B.dg_ref_of(g, D)
    dx = ref['dx'].v.reshape(c.N, g.per, c.C)
    assert rel(dx[:, :g.Tp], tm['dxp']) <= 1e-12
    assert (ref['dx'].a >= np.abs(ref['dx'].v) * (1 - 1e-15)).all() and ref['dx'].d == g.Kw * g.Cout
    assert rel(ref['sums'].v[0], tm['dbeta']) <= 1e-12
    if c.bn1:
        assert rel(ref['sums'].v[1], tm['dgamma']) <= 1e-12           # sum g xhat with xhat = (y - mean) invstd IS d gamma
    else:
        assert not ref['sums'].v[1].any() and not ref['sums'].a[1].any()
    assert (ref['sums'].a >= np.abs(ref['sums'].v) * (1 - 1e-15)).all()
    # exact accumulators as the source: the same values, the bound of the epilogue alone
    alone = B.dg_ref_of(g, D, dx=ref['dx'].v)
    assert np.array_equal(alone.v, ref['sums'].v) and alone.d == ref['sums'].d - g.Kw * g.Cout
    assert (alone.bound() <= ref['sums'].bound()).all()


@pytest.mark.parametrize('g', TORCH_CASES + B.DG_CASES, ids=lambda g: g.name)
def test_fold_first_equals_row_by_row(g):
    """the reference folds the halo rows onto their frames and gates the frames; counting every padded row with its source
    frame's gate (what the kernel does, and the form the planted defects are written in) gives the same sums: linearity.
    Here the whole buffer is random, so the dead rows of dx are not zero -- and must not count."""
    c = g.u
    D = B.make_dg_case(g)
    ref = B.dg_ref_of(g, D)
    rows = B._rowwise_sums(ref['dx'], g.per, c.N, c.T, c.C, D['y'], D['scale'], D['shift'], D['mean'], D['invstd'], c.act, c.p,
                           D['mask'], D['lens'], c.pad_l, c.pad_r, c.pad_mode, None)
    assert ratio(rows.v, ref['sums'].v, 1e-12 * ref['sums'].a + 1e-300) <= 1
    assert ratio(rows.a, ref['sums'].a, 1e-12 * ref['sums'].a + 1e-300) <= 1
    if g.per > g.Tp:
        dead = ref['dx'].v.reshape(c.N, g.per, c.C)[:, g.Tp:]
        assert np.abs(dead).min(axis=(0, 1)).max() > 0 and (np.abs(dead).sum((0, 1)) > 0).all()


def test_plain_sources_unchanged_by_the_tracked_form():
    """a tracked source of depth 0 whose magnitude is |value| is the plain array"""
    c = B.GENERAL[0]
    D = B.make_case(c)
    g, pl, pr, pm = D['srcs'][0]
    args = (c.N, c.T, c.C, D['y'], D['scale'], D['shift'], D['mean'], D['invstd'])
    kw = dict(act=c.act, p=c.p, mask=D['mask'], lens=D['lens'])
    plain = B.bn_act_bwd_ref(*args, [(g, pl, pr, pm)], **kw)
    tracked = B.bn_act_bwd_ref(*args, [(B.Tr(g), pl, pr, pm)], **kw)
    for k in ('sums', 'dy'):
        assert np.array_equal(plain[k].v, tracked[k].v) and np.array_equal(plain[k].a, tracked[k].a) and plain[k].d == tracked[k].d
    deep = B.bn_act_bwd_ref(*args, [(B.Tr(g, 2 * np.abs(g), 5), pl, pr, pm)], **kw)
    assert deep['sums'].d == plain['sums'].d + 5 and np.allclose(deep['sums'].a[0], 2 * plain['sums'].a[0])


@pytest.mark.parametrize('g', B.DG_CASES, ids=lambda g: g.name)
def test_gpu_case_conditions(g):
    c = g.u
    D = B.make_dg_case(g)
    assert not B.gate_ambiguous(c, D).any(), 'gates must be equal, not approximately equal'
    assert g.Kw * g.Cout + c.N * g.Tp + 8 < 5000, "Tr.bound's range"
    assert c.C % 64 == 0 and g.Cout in (128, 192) and g.Kw <= 7 and 450 <= g.flat_rows <= 1000 and g.halo >= g.hb
    assert g.flat_rows == c.N * g.per and g.per >= g.Tp and D['dy'].shape == (g.halo + g.flat_rows, g.Cout)
    assert c.pad_mode == 0 or (c.pad_l < c.T and c.pad_r < c.T)


def test_gpu_cases_are_what_they_are_named_for():
    A, Bc, Cc, Dc, E = B.DG_CASES
    assert A.per == A.Tp == 153 and A.u.C % 128 == 64 and A.per % 16 != 0
    assert Bc.per == 192 and Bc.per > Bc.Tp and Bc.halo == B.engine_halo(Bc.Tout, Bc.hb)
    assert Cc.u.pad_mode == 0 and Cc.u.act == 2 and Cc.u.p == 0 and Cc.u.lens == 'none' and Cc.u.C == 320
    assert Dc.u.pad_mode == 1 and Dc.u.T - 1 == Dc.u.pad_r
    assert E.u.bn1 == 0
    for g in B.DG_CASES:
        lens = B.make_dg_case(g)['lens']
        assert g.u.lens == 'none' or (0 in lens and g.u.T in lens)


@pytest.mark.parametrize('defect', B.DG_DEFECTS)
def test_defects_exceed_the_bound_of_every_gpu_case_they_apply_to(defect):
    """proved here, without a GPU: a kernel with this defect cannot pass a GPU case the defect can show on.  Case B (the engine's
    geometry: reflect, dead rows, dropout, ragged lens) shows every one of them."""
    shown = []
    for g in B.DG_CASES:
        D = B.make_dg_case(g)
        good, bad = B.dg_ref_of(g, D)['sums'], B.dg_ref_of(g, D, defect=defect)['sums']
        r = ratio(bad.v, good.v, good.bound())
        if B.dg_defect_applies(g, defect):
            assert r > 1, (g.name, defect, r)
            assert ratio(good.v, bad.v, bad.bound()) > 1, (g.name, defect)      # the GPU test's form: against the defect's bound
            shown.append(g.name)
        else:
            assert ratio(bad.v, good.v, 1e-12 * good.a + 1e-300) <= 1, (g.name, defect, 'the defect has nothing to act on here')
    assert B.DG_B.name in shown, shown
