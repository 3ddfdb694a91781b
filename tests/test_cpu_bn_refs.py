"""The float64 references of tests/bn_refs.py pinned (no GPU): Philox4x32-10 against the published known answers, the e4m3
encoder against torch.float8_e4m3fn, the forward / backward references against torch float64 autograd, the statistics finalize
against torch.nn.BatchNorm1d -- and the bounds shown to have teeth: every planted defect exceeds its bound somewhere on the shared
cases.  The conditions the GPU tests lean on are asserted for every shared case: no gate-ambiguous element, no clip-ambiguous
element, every clamp outcome well represented, buffer sizes as the launchers' formulas give them."""
import dataclasses

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bn_refs as B
from bn_refs import Case
from direct_helpers import ratio

EPS = 1e-3


def by_name(name):
    return next(c for c in B.ALL_CASES if c.name == name)


# ---- Philox, e4m3 --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('ctr,key,want', [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
])
def test_philox_known_answers(ctr, key, want):
    assert tuple(int(w) for w in B.philox4x32_10(ctr, key)) == want
    vec = B.philox4x32_10([np.array([c, c]) for c in ctr], key)          # vectorised form
    assert all(int(w[1]) == x for w, x in zip(vec, want))


def test_keep_bits_layout():
    seed, offset, gidx = 0x0123456789ABCDEF, (5 << 32) | 7, np.array([3, (9 << 32) | 1], dtype=np.uint64)
    for p in (0.3, 0.5):
        th = int(np.float32(p) * np.float32(65536))
        got = B.keep_bits(seed, offset, gidx, p)
        for i, g in enumerate(gidx.tolist()):
            w = B.philox4x32_10((g & 0xFFFFFFFF, g >> 32, 7, 5), (0x89ABCDEF, 0x01234567))
            u16 = [h for x in w for h in (int(x) & 0xFFFF, int(x) >> 16)]
            assert int(got[i]) == sum((u >= th) << j for j, u in enumerate(u16))
    assert B.keep_threshold(0.3) == 19660 and B.keep_threshold(0.5) == 32768 and B.keep_threshold(0.5, 'thresh65535') == 32767


def test_e4m3_against_torch():
    vals = B.E4M3[np.isfinite(B.E4M3)]
    assert np.array_equal(B.E4M3[np.isfinite(B.E4M3)], torch.arange(256, dtype=torch.uint8).view(torch.float8_e4m3fn).double().numpy()[
        np.isfinite(B.E4M3)])
    pos = np.sort(vals[vals >= 0])
    mid = (pos[1:] + pos[:-1]) / 2
    x = np.concatenate([pos, mid, np.nextafter(mid.astype(np.float32), 0), np.nextafter(mid.astype(np.float32), 1e9), [448.0, 464.0, 1e6]])
    x = np.concatenate([x, -x]).astype(np.float32)
    want = torch.from_numpy(x).clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8).numpy()
    got = B.e4m3_rne_sat(x.astype(np.float64))
    nz = x != 0
    assert np.array_equal(got[nz], want[nz])
    assert set(got[~nz].tolist()) <= {0x00, 0x80}


def test_quantize_dyn_ref():
    for a, s in ((224.0, 1.0), (112.0, 2.0), (448.0, 0.5), (7.0, 32.0), (1.75, 128.0), (224.0 * 2.0 ** -20, 2.0 ** 20)):
        assert B.quantize_dyn_ref([0.0, a, a / 3]) == (s, 1 / s)
        up, dn = float(np.nextafter(np.float32(a), np.float32(1e9))), float(np.nextafter(np.float32(a), np.float32(0)))
        assert B.quantize_dyn_ref([up])[0] == s / 2 and B.quantize_dyn_ref([dn])[0] == s
    assert B.quantize_dyn_ref(np.zeros(64)) == (1.0, 1.0)


# ---- torch float64 autograd ------------------------------------------------------------------------------------------------------

def torch_model(c, D):
    """forward and backward of the unit in torch float64; BatchNorm in train mode on the case's y.  Returns what the references
    return, and the float64 statistics to feed them with."""
    N, T, Cc = c.N, c.T, c.C
    rng = np.random.default_rng(7)
    t64 = lambda v: torch.from_numpy(np.asarray(v, dtype=np.float64))
    st = {}

    def bn(yk, k, on):
        x = t64(D[yk]).transpose(1, 2).contiguous().requires_grad_(True)                # [N][C][T]
        if not on:
            return x, x, None, None
        ga, be = t64(rng.random(Cc) + 0.5).requires_grad_(True), t64(rng.standard_normal(Cc)).requires_grad_(True)
        y64 = D[yk].astype(np.float64)
        mean, inv = y64.mean((0, 1)), 1 / np.sqrt(y64.var((0, 1)) + EPS)
        st.update({'mean' + k: mean, 'invstd' + k: inv, 'scale' + k: ga.detach().numpy() * inv,
                   'shift' + k: be.detach().numpy() - mean * ga.detach().numpy() * inv})
        return x, F.batch_norm(x, None, None, ga, be, training=True, eps=EPS), ga, be

    x1, z, ga1, be1 = bn('y', '', c.bn1)
    x2 = ga2 = be2 = None
    if c.res:
        x2, z2, ga2, be2 = bn('y2', '2', c.res == 1)
        z = z + z2
    if c.p > 0:
        keep = torch.from_numpy(B.unpack_keep(D['mask'], N, T, Cc)).transpose(1, 2).double()
        z = z * keep * B.inv_keep_f32(c.p)
    a = z.clamp(0, 20) if c.act == 1 else (F.relu(z) if c.act == 2 else z)
    if D['lens'] is not None:
        a = a.masked_fill(torch.arange(T)[None, None, :] >= torch.from_numpy(D['lens'].astype(np.int64))[:, None, None], 0.0)
    pad = lambda pl, pr, pm: F.pad(a, (pl, pr), mode='reflect' if pm == 1 else 'constant')
    out = F.pad(pad(c.pad_l, c.pad_r, c.pad_mode), (0, c.tail))
    loss = 0
    for g, pl, pr, pm in D['srcs']:
        rows = pl + T + pr
        loss = loss + (pad(pl, pr, pm) * t64(g[:, :rows]).transpose(1, 2)).sum()
    loss.backward()
    lay = lambda x: None if x is None else x.grad.transpose(1, 2).numpy()
    return dict(out=out.detach().transpose(1, 2).numpy(), dy=lay(x1), dy2=lay(x2), st=st,
                dbeta=None if be1 is None else be1.grad.numpy(), dgamma=None if ga1 is None else ga1.grad.numpy(),
                dgamma2=None if ga2 is None else ga2.grad.numpy())


CPU_GATES = [Case('cpu_gate_clamp', 2, 9, 8, bn1=0, act=1, pad_l=2, pad_r=2, pad_mode=1, seed=61),
             Case('cpu_gate_relu', 2, 9, 8, bn1=0, act=2, seed=62)]
TORCH_CASES = [c for c in B.ALL_CASES if not B.is_big(c)] + CPU_GATES


def rel(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


@pytest.mark.parametrize('c', TORCH_CASES, ids=lambda c: c.name)
def test_refs_match_torch_float64(c):
    D = dict(B.make_case(c))
    tm = torch_model(c, D)
    D.update(tm['st'])                                  # float64 statistics, as torch has them
    N, T, Cc = c.N, c.T, c.C
    fw = B.fwd_ref_of(c, D)
    assert rel(fw['a'].v, tm['out']) <= 1e-12
    assert (fw['a'].a >= np.abs(fw['a'].v) * (1 - 1e-15)).all()
    bw = B.bwd_ref_of(c, D, halo=3, halo2=1)

    def frames(tr, h):
        v = tr.v.reshape(-1, Cc)
        idx = np.concatenate([np.arange(h + n * (T + h), h + n * (T + h) + T) for n in range(N)])
        rest = np.setdiff1d(np.arange(v.shape[0]), idx)
        assert not v[rest].any() and not tr.a[rest].any(), 'halo rows are zero'
        return v[idx].reshape(N, T, Cc)

    dy = frames(bw['dy'], 3)
    assert rel(dy, tm['dy']) <= 1e-12
    if c.bn1:
        assert rel(bw['sums'].v[0], tm['dbeta']) <= 1e-12 and rel(bw['sums'].v[1] * 1.0, tm['dgamma'] * D['invstd'] / D['invstd']) <= 1e-10
        assert (np.abs(dy.sum((0, 1))) <= 1e-12 * np.abs(dy).sum((0, 1)) + 1e-300).all(), 'sum(dy) == 0 under BatchNorm'
    if c.res:
        assert rel(frames(bw['dy2'], 1), tm['dy2']) <= 1e-12
        if c.res == 1:
            assert rel(bw['sums'].v[3], tm['dgamma2']) <= 1e-10
            assert np.array_equal(bw['sums'].v[2], bw['sums'].v[0])
    if c.name.startswith('cpu_gate'):                   # z = y exactly: the planted 0 and 20 sit ON the gates' edges
        z = D['y'][:, :, :4]
        g = B.fold_grad(D['srcs'][0][0], N, T, Cc, c.pad_l, c.pad_r, c.pad_mode)[0][:, :, :4]
        open_ = (z >= 0) & (z <= 20) if c.act == 1 else z > 0
        assert (z == 0).any() and (z == 20).any()
        assert np.array_equal(dy[:, :, :4], np.where(open_, g, 0.0))


@pytest.mark.parametrize('count_rows', [(1, 1), (7, 5), (121, 5)])
def test_finalize_ref_matches_batchnorm1d(count_rows):
    rows, per = count_rows
    Cc = 40
    rng = np.random.default_rng(5)
    x = (rng.standard_normal((rows * per, Cc)) * 2 + 1).astype(np.float32).astype(np.float64)
    pr = np.stack([x.reshape(rows, per, Cc).sum(1), (x.reshape(rows, per, Cc) ** 2).sum(1)], axis=1)
    bn = torch.nn.BatchNorm1d(Cc, eps=EPS, momentum=0.25).double()
    with torch.no_grad():
        bn.weight.copy_(torch.from_numpy(rng.random(Cc) + 0.5))
        bn.bias.copy_(torch.from_numpy(rng.standard_normal(Cc)))
        bn.running_mean.copy_(torch.from_numpy(rng.standard_normal(Cc)))
        bn.running_var.copy_(torch.from_numpy(rng.random(Cc) + 0.5))
    rm, rv = bn.running_mean.numpy().copy(), bn.running_var.numpy().copy()
    ga, be = bn.weight.detach().numpy(), bn.bias.detach().numpy()
    xt = torch.from_numpy(x)
    if rows * per > 1:
        want = bn.train()(xt).detach().numpy()
        r = B.bn_finalize_ref(pr, Cc, rows * per, ga, be, EPS, 0.25, rm, rv)
        assert rel(x * r['scale'].v + r['shift'].v, want) <= 1e-9          # (E[x^2] - mu^2 cancels a few digits)
        assert rel(r['running_mean'].v, bn.running_mean.numpy()) <= 1e-12
        assert rel(r['running_var'].v, bn.running_var.numpy()) <= 1e-9
        assert rel((x - r['mean'].v) * r['invstd'].v, (want - be) / ga) <= 1e-9
    else:                                               # one element: the unbiased variance equals the biased one (0)
        r = B.bn_finalize_ref(pr, Cc, 1, None, None, EPS, 0.25, rm, rv)
        assert rel(r['running_var'].v, 0.75 * rv) <= 1e-12 and rel(r['invstd'].v, np.full(Cc, 1 / np.sqrt(B.f32(EPS)))) <= 1e-9
        assert np.array_equal(r['scale'].v, r['invstd'].v)
    rm2, rv2 = bn.running_mean.numpy().copy(), bn.running_var.numpy().copy()
    ev = B.bn_finalize_ref(None, Cc, 0, ga, be, EPS, 0.25, rm2, rv2)
    assert rel(x * ev['scale'].v + ev['shift'].v, bn.eval()(xt).detach().numpy()) <= 1e-9   # (eps: float32(1e-3) here)
    assert set(ev) == {'mean', 'invstd', 'scale', 'shift'}


# ---- the conditions the GPU tests lean on ------------------------------------------------------------------------------------------

@pytest.mark.parametrize('c', B.ALL_CASES, ids=lambda c: c.name)
def test_case_conditions(c):
    D = B.make_case(c)
    N, T, Cc = c.N, c.T, c.C
    assert not B.gate_ambiguous(c, D).any(), 'an element whose gate float64 and fp32 could decide differently'
    assert D['resampled'] <= 1e-5 * N * T * Cc + 2, 'resampling is a safeguard, not a crutch'
    z = B.z_prime(c, D).v
    assert (z[:, :, :4] == 0).any(), 'planted: z exactly 0'
    if c.p == 0:
        assert (z[:, :, :4] == 20).any(), 'planted: z exactly 20'
    if c.act == 1:
        shares = [(z < 0).mean(), ((z >= 0) & (z <= 20)).mean(), (z > 20).mean()]
        assert min(shares) >= 0.05, shares
    if c.q_scale:
        fw = B.fwd_ref_of(c, D)
        assert not (np.abs(fw['clip_margin']) <= fw['clip_bound']).any()
        assert 0.002 * N * T * Cc <= fw['clipped'] <= 0.03 * N * T * Cc, fw['clipped']
    # sizes, from the formulas of include/w2l_hip.h
    s = c.sizes(halo=13, halo2=1)
    R = c.pad_l + T + c.pad_r + c.tail
    assert s['out'] == N * R * Cc and s['mask'] * 8 == N * T * Cc and s['dy'] == (13 + N * (T + 13)) * Cc
    assert s['dy2'] == (1 + N * (T + 1)) * Cc and s['amax'] == 2 * 64 and s['src1'] == N * R * Cc
    for g, pl, pr, pm in D['srcs']:
        assert g.shape[0] == N and g.shape[1] >= pl + T + pr and g.shape[2] == Cc
        assert pm != 1 or (pl < T and pr < T)
    if Cc % 64 == 0:
        rw = B.bwd_rows_per_wave(N * T, Cc)
        assert rw % 8 == 0 and 16 <= rw <= 64 and s['partial'] == -(-N * T // rw) * (4 if c.res else 2) * Cc
    assert N * R * (Cc // 8) < 2 ** 31 and R * (Cc // 8) < 2 ** 24


def test_shapes_reach_the_paths_they_are_named_for():
    assert [B.bwd_rows_per_wave(c.N * c.T, c.C) for c in map(by_name, ('clamp', 'mid_rows', 'wide_rows'))] == [16, 24, 64]
    assert all((c.N * c.T) % B.bwd_rows_per_wave(c.N * c.T, c.C) for c in map(by_name, ('clamp', 'mid_rows', 'wide_rows')))
    assert B.apply_rows_per_block(111, 64) == 64 and B.apply_rows_per_block(8 * 1825, 1024) == 160
    assert [B.bn_loop_iters(c.N * c.T, c.T, c.C) for c in B.LOOPED] == [4, 4, 0, 0]
    assert B.LOOPED[2].N * B.LOOPED[2].T >= 12000 and B.LOOPED[2].T < 8 and B.LOOPED[3].N * B.LOOPED[3].T == 11983
    c = B.BIG_APPLY
    assert (c.N * c.T + 40 * (c.N + 1)) * c.G > 4096 * 256
    c = B.FWD_FIN_BIG
    assert c.N * c.R * (c.C // 64) > 81920 and B.fwd_rows_per_block(c.N * c.R, c.C) == 64
    assert B.fwd_rows_per_block(B.FWD_FIN_SMALL.N * B.FWD_FIN_SMALL.R, 128) == 32
    c = by_name('ragged_grid')
    assert c.R * c.G == 2 * 256 + 1
    assert B.general_sum_depth(5, 1031, 960, 'finalize') < 5000 and B.slots_sum_depth(24, 500, 704, 1, 1) < 5000


# ---- teeth ---------------------------------------------------------------------------------------------------------------------

def dy_ratio(name, defect, key='dy', r_out=B.R_BF16):
    c = by_name(name)
    D = B.make_case(c)
    good, bad = B.bwd_ref_of(c, D, halo=1, halo2=1), B.bwd_ref_of(c, D, halo=1, halo2=1, defect=defect)
    return ratio(bad[key].v, good[key].v, good[key].bound(r_out))


@pytest.mark.parametrize('name,defect,key', [
    ('clamp', 'gate_open_20', 'dy'), ('relu_res_nobn2_f32y', 'relu_closed_0', 'dy'), ('clamp_f32_drop_lens', 'no_inv_keep_grad', 'dy'),
    ('clamp_f32_drop_lens', 'masked_xhat_dropped', 'dy'), ('clamp', 'fold_right_T2', 'dy'), ('clamp', 'sum_g_M1', 'dy'),
    ('relu_res_drop_two', 'res_sumgx_xhat1', 'dy2'), ('relu_res_drop_two', 'res_sumgx_xhat1', 'sums'),
    ('clamp', 'gate_open_20', 'sums'), ('u1', 'no_inv_keep_grad', 'sums'), ('u1', 'fold_right_T2', 'dy'),
])
def test_backward_defects_exceed_the_bound(name, defect, key):
    assert dy_ratio(name, defect, key, 0.0 if key == 'sums' else B.R_BF16) > 1


def test_forward_defects_exceed_the_bound():
    c = by_name('clamp')
    D = B.make_case(c)
    good, bad = B.fwd_ref_of(c, D), B.fwd_ref_of(c, D, defect='tail_unwritten')
    assert ratio(bad['a'].v, good['a'].v, good['a'].bound(B.R_BF16)) > 1
    c = by_name('c8')
    D = B.make_case(c)
    good, bad = B.fwd_ref_of(c, D), B.fwd_ref_of(c, D, defect='halo_fresh_bits')
    assert ratio(bad['a'].v, good['a'].v, good['a'].bound(B.R_BF16)) > 1
    assert np.array_equal(good['mask'], bad['mask'])
    # the keep threshold: p = 0.5 is 32768 of 65536; p * 65535 truncates to 32767 and keeps the elements that drew exactly that
    c = by_name('loop_t8')
    gidx = np.arange(c.N * c.T * c.G, dtype=np.uint64)
    assert (B.keep_bits(1, 2, gidx, c.p) != B.keep_bits(1, 2, gidx, c.p, 'thresh65535')).sum() > 10


def test_finalize_defect_exceeds_the_bound():
    pr, count = B.make_partial(121, 40, 5, 3)
    rng = np.random.default_rng(1)
    args = (pr, 40, count, rng.random(40).astype(np.float32) + 0.5, rng.standard_normal(40).astype(np.float32), EPS, 0.1, None, None)
    good, bad = B.bn_finalize_ref(*args), B.bn_finalize_ref(*args, defect='unbiased_invstd')
    for k in ('invstd', 'scale', 'shift'):
        assert ratio(bad[k].v, good[k].v, good[k].bound()) > 1
    assert good['invstd'].d == 1 and good['scale'].d == 2              # a few u relative
