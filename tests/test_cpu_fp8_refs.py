"""The float64 references of the e4m3 kernels (tests/fp8_refs.py, used by tests/test_gpu_fp8_direct.py) pinned on the CPU:
against torch float64 (autograd of F.conv1d for the weight gradient, F.conv1d for the convolution); the exactness arithmetic of
the exact family asserted per case (every sum an integer below 2^24 units of the result's unit); every planted defect shown to
change a bit of the exact family wherever it applies -- and nothing where it does not -- and to lie outside the full-range
bound (F8_DOT_MARGIN included) on at least one case; the operand layouts the GPU test relies on (zero dy rows, NaN codes where
nothing may be read, live x bytes beneath the dead frames); every path of conv_wgrad_fp8.hip named in WGRAD8_PATHS reached by the
case that is there for it; and the table of which (case, block shape, statistics flag) runs pinned to the host-only plan query."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_refs as C
import fp8_refs as R
from direct_helpers import ratio
from fp8_refs import CONV8_CASES, E4M3, FAMILIES, FUSED8_CASES, NAN8, U, WGRAD8_CASES, WGRAD8_DEFECTS


def rel(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def t64(a):
    return torch.from_numpy(np.array(a, dtype=np.float64, order="C"))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def test_operand_families():
    rng = np.random.default_rng(0)
    ex = E4M3[R.codes_exact(rng, (4096,))]
    assert set(ex.tolist()) == set(range(-4, 5))
    full = R.codes_full(rng, (1 << 16,))
    assert len(set(full.tolist())) == 254 and np.isfinite(E4M3[full]).all() and np.abs(E4M3[full]).max() == 448
    assert (E4M3[full] == 2.0 ** -9).any() and 0x80 in full and np.isnan(E4M3[NAN8])
    want = torch.from_numpy(np.arange(256, dtype=np.uint8)).view(torch.float8_e4m3fn).double().numpy()
    assert np.array_equal(np.nan_to_num(want, nan=7e7), np.nan_to_num(E4M3, nan=7e7))
    for fam in FAMILIES:
        for f in R.FACTORS[fam]:
            m, _ = np.frexp(f)
            assert (m == 0.5) == (fam == 'exact') and float(np.float32(f)) == f
    assert R.EXACT_UNIT == R.FACTORS['exact'][0] * R.FACTORS['exact'][1] and R.F8_DOT_MARGIN == 32


# ---- A. the weight gradient ----------------------------------------------------------------------------------------------------------

def autograd_dw(c, D):
    x = t64(np.stack([E4M3[D['x']][n * c.per: n * c.per + c.need] for n in range(c.N)])).transpose(1, 2)
    dy = t64(E4M3[D['dy'][c.hb:]].reshape(c.N, c.dy_per, c.Cout)[:, :c.T]).transpose(1, 2)
    w = torch.zeros(c.Cout, c.Cin, c.Kw, dtype=torch.float64, requires_grad=True)
    y = F.conv1d(x, w, None, dilation=c.dil)
    assert y.shape == (c.N, c.Cout, c.T)
    y.backward(dy)
    return w.grad.permute(2, 0, 1).numpy()


@pytest.mark.parametrize('fam', FAMILIES)
@pytest.mark.parametrize('c', WGRAD8_CASES, ids=lambda c: c.name)
def test_wgrad8_ref_matches_torch_float64_autograd(c, fam):
    D = R.make_wgrad8_case(c, fam)
    want = autograd_dw(c, D)
    S, A = R.wgrad8_sums(c, D)
    assert S.shape == (c.Kw, c.Cout, c.Cin) and rel(S, want) <= 1e-12 and (A >= np.abs(S) * (1 - 1e-15)).all()
    ds, dd = R.FACTORS[fam]
    for acc in (False, True):
        for dev in (False, True):
            for splits in (1, c.max_splits):
                v, b = R.wgrad8_ref(c, D, splits, acc, dev)
                full = want * ds * (dd if dev else 1.0) + (D['dw0'].astype(np.float64) if acc else 0.0)
                assert rel(v, full) <= 1e-12
                Ab = A * ds * (dd if dev else 1.0) + (np.abs(D['dw0']) if acc else 0.0)
                assert np.allclose(b, (R.F8_DOT_MARGIN * c.K + dev + 1 + splits - 1 + acc) * U * Ab, rtol=1e-12, atol=0)
    if fam == 'exact':
        # the exactness arithmetic: every sum of products is an integer, the whole result a multiple of the unit below 2^24 units
        assert np.array_equal(S, np.rint(S)) and np.abs(S).max() <= 16 * c.K
        assert R.exact_units(c.K) < 2 ** 16 < 2 ** 24 and A.max() <= 16 * c.K
        dw0 = D['dw0'].astype(np.float64)
        assert np.array_equal(dw0 * 16, np.rint(dw0 * 16)) and np.abs(dw0).max() < 2 ** 10
        v, _ = R.wgrad8_ref(c, D, c.max_splits, True, True)
        assert np.array_equal(v / R.EXACT_UNIT, np.rint(v / R.EXACT_UNIT)) and np.abs(v / R.EXACT_UNIT).max() <= R.exact_units(c.K)
        assert np.array_equal(v.astype(np.float32).astype(np.float64), v)
        # ... so a sequential fp32 sum of one element, in reverse order, scaled and accumulated in fp32, has the reference's bits
        dyv = E4M3[D['dy'][c.hb:]].reshape(c.N, c.dy_per, c.Cout)
        acc32 = np.float32(0)
        for n in reversed(range(c.N)):
            for t in reversed(range(c.T)):
                acc32 = np.float32(acc32 + np.float32(dyv[n, t, -1] * E4M3[D['x'][n * c.per + t + (c.Kw - 1) * c.dil, -1]]))
        got = np.float32(np.float32(acc32 * np.float32(ds * dd)) + D['dw0'][-1, -1, -1])
        assert bits(got) == bits(v[-1, -1, -1])


@pytest.mark.parametrize('fam', FAMILIES)
@pytest.mark.parametrize('c', WGRAD8_CASES, ids=lambda c: c.name)
def test_wgrad8_operand_layout(c, fam):
    """what the GPU test relies on: zero codes in the dead dy rows, the NaN code in every dy row no step covers, finite live codes
    in EVERY x row (the rows beneath dead frames, gap rows and the tail included: most of them non-zero), a dy stride that holds
    every step, the key of the tune cache used by no other test of the suite"""
    D = R.make_wgrad8_case(c, fam)
    x, dy = D['x'], D['dy']
    assert x.shape == (c.x_rows_total, c.Cin) and x.dtype == np.uint8 and np.isfinite(E4M3[x]).all()
    assert (E4M3[x] != 0).mean(1).min() > 0.5 or c.x_rows_total == 1
    assert dy.shape == (c.hb + c.N * c.dy_per, c.Cout) and c.dy_per >= c.tsteps * 128 and c.dy_per - c.T >= c.hb
    dv = dy[c.hb:].reshape(c.N, c.dy_per, c.Cout)
    assert (dy[:c.hb] == NAN8).all() and np.isfinite(E4M3[dv[:, :c.T]]).all()
    assert not dv[:, c.T: c.tsteps * 128].any() and (dv[:, c.tsteps * 128:] == NAN8).all()
    if c.x_tail == 0:
        assert c.x_rows_total == (c.N - 1) * c.per + c.T + (c.Kw - 1) * c.dil      # ends at the last row a live product reads
    others = [(3, 128, 256, 333, 5), (2, 256, 128, 500, 1), (2, 192, 320, 200, 4), (4, 384, 256, 500, 11), (1, 128, 128, 75, 29),
              (2, 128, 128, 130, 3)]                                                # tests/test_gpu_fp8.py
    assert c.key not in others
    assert R.tune_line(c, 3, 1) == 'wgradf8 %d %d %d %d %d 3 1\n' % c.key


def test_wgrad8_cases_reach_what_they_are_there_for():
    reached = set()
    for c in WGRAD8_CASES:
        p = R.wgrad8_paths(c)
        assert p >= R.WGRAD8_CASE_PATHS[c.name], (c.name, R.WGRAD8_CASE_PATHS[c.name] - p)
        reached |= p
    assert reached == set(R.WGRAD8_PATHS), set(R.WGRAD8_PATHS) ^ reached
    W1, W2, W3, W4, W5, W6 = WGRAD8_CASES
    assert (W1.tsteps, W1.tsteps * 128 - W1.T, W1.Kw % 2, W1.Cout % 128, W1.Cin) == (2, 126, 1, 64, 64)
    assert (W2.steps, W2.T, W2.kwb, W2.max_splits) == (1, 1, 1, 1)
    assert (W3.T % 128, W3.xrows, W3.dil % 2) == (0, 160, 0)
    assert (W4.steps, W4.T - 2 * 128, W4.dil % 2, W4.max_splits) == (15, 1, 1, 15)
    assert (128 + W5.dil, W5.xrows, W5.xrows // 8 % 4) == (145, 152, 3)
    assert W6.key == W1.key and W6.gap == 0 and W6.x_tail == 0 and W6.per == W6.T + W6.hb and W1.gap > 0
    # W4: splits whose steps_per_split rounds up, splits with idle trailing blocks, blocks that cross utterances
    sps = {s: -(-15 // s) for s in range(1, 16)}
    assert sum(sps[s] * s > 15 and sps[s] > 1 for s in sps) >= 5 and sum((s - 1) * sps[s] >= 15 for s in sps) >= 5
    assert [len(R.wgrad8_plans(c)) for c in WGRAD8_CASES] == [12, 2, 4, 30, 4, 12]


def _launch_forms(c):
    return [(s, acc, dev) for s in sorted({1, 2, c.max_splits} & set(range(1, c.max_splits + 1))) for acc in (False, True)
            for dev in (False, True)]


@pytest.mark.parametrize('c', WGRAD8_CASES, ids=lambda c: c.name)
def test_every_wgrad8_defect_changes_a_bit_of_the_exact_family(c):
    D = R.make_wgrad8_case(c, 'exact')
    for splits, acc, dev in _launch_forms(c):
        good, _ = R.wgrad8_ref(c, D, splits, acc, dev)
        for name in WGRAD8_DEFECTS:
            bad, _ = R.wgrad8_ref(c, D, splits, acc, dev, defect=name)
            if R.wgrad8_defect_applies(c, name, splits, acc, dev):
                assert not np.array_equal(bits(bad), bits(good)), (c.name, name, splits, acc, dev)
            else:
                assert np.array_equal(bad, good), (c.name, name, 'acts where it is said not to')


FULL_SHOWN = {}


@pytest.mark.parametrize('c', WGRAD8_CASES, ids=lambda c: c.name)
def test_wgrad8_defects_against_the_full_range_bound(c):
    """per case: which defects lie outside the full-range bound, both ways round (the form the GPU test asserts); a right result
    stays inside"""
    D = R.make_wgrad8_case(c, 'full')
    for splits, acc, dev in _launch_forms(c):
        good, gb = R.wgrad8_ref(c, D, splits, acc, dev)
        assert ratio(good.astype(np.float32), good, gb) <= 1
        for name in WGRAD8_DEFECTS:
            if R.wgrad8_defect_applies(c, name, splits, acc, dev):
                bad, bb = R.wgrad8_ref(c, D, splits, acc, dev, defect=name)
                if ratio(bad, good, gb) > 1 and ratio(good, bad, bb) > 1:
                    FULL_SHOWN.setdefault(name, set()).add(c.name)


def test_every_wgrad8_defect_lies_outside_the_full_range_bound_somewhere():
    if len(FULL_SHOWN) == 0:
        for c in WGRAD8_CASES:
            test_wgrad8_defects_against_the_full_range_bound(c)
    assert set(FULL_SHOWN) == set(WGRAD8_DEFECTS), set(WGRAD8_DEFECTS) - set(FULL_SHOWN)
    for name in WGRAD8_DEFECTS:
        assert any(R.wgrad8_defect_applies(c, name, s, True, True) for c in WGRAD8_CASES for s, _ in R.wgrad8_plans(c)), name


# ---- B. the convolution --------------------------------------------------------------------------------------------------------------

def torch_conv(c, D, flipped, bias, dev):
    x = t64(E4M3[D['x']][:c.N * c.per].reshape(c.N, c.per, c.Cin)[:, :c.need]).transpose(1, 2)
    w = E4M3[D['w']]
    ds, dd = R.FACTORS[D['family']]
    y = F.conv1d(x, t64(w[:, :, ::-1] if flipped else w), None, dilation=c.dil).transpose(1, 2).numpy() * ds * (dd if dev else 1.0)
    return y + (D['bias'].astype(np.float64) if bias else 0.0)


@pytest.mark.parametrize('fam', FAMILIES)
@pytest.mark.parametrize('c', CONV8_CASES, ids=lambda c: c.name)
def test_conv8_ref_matches_torch_float64(c, fam):
    D = R.make_conv8_case(c, fam)
    assert c.stride == 1 and c.Cin % 128 == 0 and np.isfinite(E4M3[D['x']]).all() and np.isfinite(E4M3[D['w']]).all()
    xv = D['x'][:c.N * c.per].reshape(c.N, c.per, c.Cin)
    assert (xv[:, c.need:] == R.SENT8).all() and (D['x'][c.N * c.per:] == R.SENT8).all()
    assert np.array_equal(R.w_device8(D)[1 % c.Kw], D['w'][:, :, 1 % c.Kw]) and np.array_equal(R.w_device8(D, True)[0], D['w'][:, :, -1])
    for flipped, bias, dev in ((False, True, True), (False, True, False), (True, False, True)):
        ref = R.conv8_ref(c, D, flipped, bias, dev)
        assert ref.v.shape == (c.N, c.Tout, c.Cout) and rel(ref.v, torch_conv(c, D, flipped, bias, dev)) <= 1e-12
        assert ref.d + 2 == R.F8_DOT_MARGIN * c.K + dev + 1 + bias and (ref.a >= np.abs(ref.v) * (1 - 1e-15)).all()
    if fam == 'exact':
        # every partial sum of the dot product is an integer below 2^16; y a multiple of 2^-5 below 2^24 units; a statistics row
        # (the sum of at most 128 columns) too, so the tile rows of s1 must have the reference's bits
        ref = R.conv8_ref(c, D)
        units = ref.v / R.EXACT_UNIT
        assert 16 * c.K < 2 ** 16 and np.array_equal(units, np.rint(units)) and np.abs(D['bias']).max() <= 64
        assert R.exact_units(c.K, added=64.0) < 2 ** 16 and np.abs(units).max() <= R.exact_units(c.K, added=64.0)
        assert 128 * R.exact_units(c.K, added=64.0) < 2 ** 24
        rows = R.tile_row_sums(c, ref.v)
        assert rows.shape == (c.N * -(-c.Tout // 128), c.Cout) and np.abs(rows / R.EXACT_UNIT).max() < 2 ** 24
        assert np.array_equal(rows.astype(np.float32).astype(np.float64), rows) and np.allclose(rows.sum(0), ref.v.sum((0, 1)))


CONV_SHOWN = {}


@pytest.mark.parametrize('c', CONV8_CASES, ids=lambda c: c.name)
def test_every_conv8_defect_is_visible(c):
    """exact family: a defect of an element changes a bit of y, a defect of the sums a bit of the tile rows' s1, wherever it can
    act, and nothing where it cannot; full range: which defects lie outside the bound, both ways round, on this case (through
    the statistics of a 128-column shape for the three that act on the sums)"""
    k = 0
    for fam in FAMILIES:
        D = R.make_conv8_case(c, fam)
        good = R.conv8_ref(c, D)
        g1, g2 = R.conv8_stats(c, D, good, k)
        for name in R.CONV8_DEFECTS:
            if name in C.ELEMENT_DEFECTS or name == 'descale_dev_ignored':
                bad = R.conv8_ref(c, D, defect=name)
                differs = ratio(bad.v, good.v, R.bound_of(good)) > 1 and ratio(good.v, bad.v, R.bound_of(bad)) > 1
                bit = not np.array_equal(bits(bad.v), bits(good.v))
            else:
                b1, b2 = R.conv8_stats(c, D, good, k, defect=name)
                differs = any(ratio(b.v, g.v, R.bound_of(g)) > 1 and ratio(g.v, b.v, R.bound_of(b)) > 1 for b, g in ((b1, g1), (b2, g2)))
                bit = not np.array_equal(b1.v, g1.v)
            if fam == 'exact':
                applies = True if name == 'last_row_dropped' else R.conv8_defect_applies(c, name)
                assert bit == applies, (c.name, name)
            elif differs:
                CONV_SHOWN.setdefault(name, set()).add(c.name)


def test_every_conv8_defect_lies_outside_the_full_range_bound_somewhere():
    if len(CONV_SHOWN) == 0:
        for c in CONV8_CASES:
            test_every_conv8_defect_is_visible(c)
    assert set(CONV_SHOWN) == set(R.CONV8_DEFECTS), (set(R.CONV8_DEFECTS) - set(CONV_SHOWN), CONV_SHOWN)


def test_conv8_shapes_and_feasibility_function():
    assert R.NF8 == 15 and len(set(R.F8_CFGS)) == 15 and 20 not in R.F8_CFGS
    assert sorted({R.f8_cols(k) for k in range(R.NF8)}) == [128, 144, 256, 288, 384, 448]
    assert sum(R.f8_fused_built(k) for k in range(R.NF8)) == 11
    assert [c.K // 128 for c in CONV8_CASES] == [5, 2, 7, 9] and F_case('F3').Tout < 128 and F_case('F1').gap > 0
    for c in CONV8_CASES:
        for flag, row in R.F8_FEASIBLE[c.name].items():
            assert ''.join(R.F8_CODE[R.f8_cannot_run(c, k, flag)] for k in range(R.NF8)) == row, (c.name, flag)
        assert R.F8_FEASIBLE[c.name][R.F8_STATS].count('r') == 9 and R.F8_FEASIBLE[c.name][R.F8_FUSED].count('r') == 11


def F_case(prefix):
    return next(c for c in CONV8_CASES if c.name.startswith(prefix))


@pytest.mark.parametrize('c', CONV8_CASES, ids=lambda c: c.name)
def test_feasibility_table_is_what_the_launcher_answers(c):
    from wav2letter_pytorch_amd import _lib as L
    out = (ctypes.c_int * 8)()
    for flag, row in R.F8_FEASIBLE[c.name].items():
        for k in range(R.NF8):
            rc = L.lib.w2l_conv_plan_fp8(c.N, c.Cin, c.Cout, c.Tout, c.Kw, c.dil, flag, k, out)
            assert (rc == 0) == (row[k] == 'r'), (c.name, flag, k, L.lib.w2l_last_error())
            if rc == 0:
                mw, nw, ms, ns = R.f8_shape(k)
                assert out[0] == k and out[2] == 1 and out[3] == 0 and out[5] == 64 * mw * nw and out[7] == 1
                assert out[4] == -(-c.Cout // (16 * mw * ms)) * c.N * -(-c.Tout // R.f8_cols(k))
            else:
                assert out[0] == -1
    assert L.lib.w2l_conv_plan_fp8(c.N, c.Cin, c.Cout, c.Tout, c.Kw, c.dil, 0, R.NF8, out) != 0


# ---- C. the fused inference epilogue -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('c', FUSED8_CASES, ids=lambda c: c.name)
def test_fused8_reference_and_defects(c):
    """the accumulator of the exact family is exact in fp32; every conv_refs.FUSED_DEFECTS that applies to a variant lies outside
    the per-element bf16 bound; the e4m3 codes the reference is certain of are most of them"""
    D = R.make_conv8_case(c, 'exact')
    names = [f.name for f, _, _ in R.fused8_variants(c)]
    assert names[:3] == ['w2l', 'jasper', 'jasper_res'] and (len(names) == 4) == (c.Kw == 1)
    shown = set()
    for f, bias, q_scale in R.fused8_variants(c):
        P = R.make_fused8_params(c, f)
        v = R.fused8_acc(c, D, bias)
        assert rel(v, torch_conv(c, D, False, bias, False)) <= 1e-12
        ref = R.fused8_ref(c, f, P, v, q_scale)
        rows = ref['rows']
        a = ref['a']
        assert a.d == 2 + (1 if f.res else 0) and np.isnan(a.v[:, rows:]).all() and np.isfinite(a.v[:, :rows]).all()
        assert f.pad_l <= 96 and f.pad_r <= 96 and (f.pad_mode == 0 or max(f.pad_l, f.pad_r) < c.Tout)
        av = a.v[:, :rows]
        assert 0.5 < np.abs(av[av != 0]).mean() < 20                     # the unit's output is O(1): the activations really act
        for name in C.FUSED_DEFECTS:
            if C.conv_defect_applies(c, name, f=f):
                bad = R.fused8_ref(c, f, P, v, q_scale, defect=name)['a']
                assert ratio(av, bad.v[:, :rows], bad.bound(C.R_BF16)[:, :rows]) > 1, (c.name, f.name, name)
                shown.add(name)
            elif name != 'res_lo_ignored':
                bad = R.fused8_ref(c, f, P, v, q_scale, defect=name)['a']
                assert np.array_equal(bad.v[:, :rows], av), (c.name, f.name, name)
        aq = ref['aq']
        codes, sure = R.e4m3_certain(np.clip(aq.v[:, :rows], -448, 448), aq.bound()[:, :rows])
        assert sure.mean() > 0.99 and np.isfinite(E4M3[codes]).all()
        assert ratio(E4M3[codes], np.clip(aq.v[:, :rows], -448, 448), R.e4m3_bound(Tr_rows(aq, rows), q_scale)) <= 1
    assert shown == {'halo_off_by_one', 'mask_before_residual', 'clamp_before_shift'} if c.Kw > 1 else shown >= {'clamp_before_shift'}


def Tr_rows(t, rows):
    return R.Tr(t.v[:, :rows], t.a[:, :rows], t.d)
