"""The float64 references of the implicit GEMM forward and of the fused inference epilogue (tests/conv_refs.py, used by
tests/test_gpu_conv_direct.py) pinned on the CPU: against torch.nn.functional.conv1d and the unfused chain in torch float64, and
every planted defect (conv_refs.CONV_DEFECTS) shown to lie outside the bound the GPU test applies to the quantity it corrupts, on
every case whose geometry lets it act -- and to change nothing where it cannot.  Case A shows all of them."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bn_refs as B
import conv_refs as R
from conv_refs import CONV_CASES, R_BF16, R_SPLIT, Tr
from direct_helpers import ratio

VARIANTS = [(c, f) for c in CONV_CASES for f in c.fused]


def rel(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def t64(a):
    return torch.from_numpy(np.asarray(a, dtype=np.float64))


def torch_conv(c, D, acc_in=False):
    """[N][Tout][Cout] float64: F.conv1d on the rows each utterance needs, + bias (+ acc_in)"""
    x = t64(R.x_view(c, D)[:, :c.need]).transpose(1, 2)
    y = F.conv1d(x, t64(D['w']), t64(D['bias']), stride=c.stride, dilation=c.dil).transpose(1, 2)
    assert y.shape == (c.N, c.Tout, c.Cout)
    return y + t64(D['acc_in']) if acc_in else y


@pytest.mark.parametrize('acc_in', [False, True], ids=['plain', 'acc_in'])
@pytest.mark.parametrize('c', CONV_CASES, ids=lambda c: c.name)
def test_conv_and_sums_match_torch_float64(c, acc_in):
    D = R.make_conv_case(c)
    y = torch_conv(c, D, acc_in).numpy()
    ref = R.conv_ref_of(c, D, acc_in=acc_in, sum_depth=5)
    v = ref['v']
    assert rel(v.v, y) <= 1e-12
    assert v.d == c.K + 1 + acc_in and (v.a >= np.abs(v.v) * (1 - 1e-15)).all()
    assert rel(ref['s1'].v, y.sum((0, 1))) <= 1e-12 and rel(ref['s2'].v, (y * y).sum((0, 1))) <= 1e-12
    assert ref['s1'].d == v.d + 5 and ref['s2'].d == 2 * v.d + 1 + 5 and ref['s2'].d < 5000, "Tr.bound's range"
    for s in (ref['s1'], ref['s2']):
        assert (s.a >= np.abs(s.v) * (1 - 1e-15)).all()
    # the epilogue-alone form: exact inputs, the chain alone
    y32 = v.v.astype(np.float32)
    a1, a2 = R.conv_stats_ref(y32, 5)
    assert a1.d == 5 and a2.d == 6 and rel(a1.a, np.abs(y32.astype(np.float64)).sum((0, 1))) <= 1e-15
    assert (a1.bound() < ref['s1'].bound()).all() and (a2.bound() < ref['s2'].bound()).all()


@pytest.mark.parametrize('c,f', VARIANTS, ids=lambda v: v.name)
def test_infer_ref_matches_torch_float64(c, f):
    D = R.make_conv_case(c)
    P = D['fused'][f.name]
    z = torch_conv(c, D, bool(f.acc_in))
    if f.affine:
        z = z * t64(P['scale']) + t64(P['shift'])
    if f.res:
        z = z + t64(P['res'])
    if f.res == 2:
        z = z + t64(P['res_lo'])
    z = z.clamp(0, 20) if f.act == 1 else (F.relu(z) if f.act == 2 else z)
    if P['lens'] is not None:
        z = z.masked_fill(torch.arange(c.Tout)[None, :, None] >= torch.from_numpy(P['lens'].astype(np.int64))[:, None, None], 0.0)
    zp = F.pad(z.transpose(1, 2), (f.pad_l, f.pad_r), mode='reflect' if f.pad_mode == 1 else 'constant').transpose(1, 2).numpy()
    ref = R.fused_ref_of(c, D, f)
    rows = f.pad_l + c.Tout + f.pad_r
    assert ref['written'].sum() == rows and ref['a'].v.shape[1] == rows + f.tail
    assert rel(ref['a'].v[:, :rows], zp) <= 1e-12 and np.isnan(ref['a'].v[:, rows:]).all()
    a = ref['a']
    assert (a.a[:, :rows] >= np.abs(a.v[:, :rows]) * (1 - 1e-15)).all()
    assert a.d == c.K + 1 + f.acc_in + 2 * f.affine + (f.res > 0) + (f.res == 2)
    # the epilogue alone, on the plain fp32 store as an exact input: 2 (affine) + 1 (acc_in) + 1 or 2 (res, res_lo) roundings
    y32 = torch_conv(c, D, False).numpy().astype(np.float32)
    alone = R.fused_ref_of(c, D, f, src=y32)['a']
    assert alone.d == f.acc_in + 2 * f.affine + (f.res > 0) + (f.res == 2) and alone.d <= 5
    assert ratio(alone.v[:, :rows], zp, a.bound(R_BF16)[:, :rows]) <= 1, 'the fp32 rounding of the store is within the full bound'
    # halo rows copy the frame the reference names
    src = ref['src']
    for r in np.nonzero(ref['written'])[0]:
        if src[r] >= 0:
            assert np.array_equal(a.v[:, r], a.v[:, f.pad_l + src[r]])
        else:
            assert not a.v[:, r].any()


def test_plain_arrays_unchanged_by_the_tracked_form():
    """bn_act_fwd_ref on the existing cases: a tracked y of depth 0 whose magnitude is |y| IS the plain array"""
    for c in B.GENERAL + B.FWD_ONLY:
        if B.is_big(c):
            continue
        D = B.make_case(c)
        plain = B.fwd_ref_of(c, D)
        D2 = dict(D, y=Tr(D['y']), y2=None if D['y2'] is None else Tr(D['y2']))
        tracked = B.fwd_ref_of(c, D2)
        assert np.array_equal(plain['a'].v, tracked['a'].v, equal_nan=True) and np.array_equal(plain['a'].a, tracked['a'].a)
        assert plain['a'].d == tracked['a'].d
        deep = B.fwd_ref_of(c, dict(D, y=Tr(D['y'], 2 * np.abs(D['y']), 7)))
        assert deep['a'].d == plain['a'].d + 7 and np.array_equal(deep['a'].v, plain['a'].v, equal_nan=True)


def test_cases_are_what_they_are_named_for():
    A, Bc, Cc, Dc, E = CONV_CASES
    for c in CONV_CASES:
        D = R.make_conv_case(c)
        assert c.K < 5000 and 2 * (c.K + 2) + 1 + R.stats_sum_depth_max(c.N, c.Tout, launches=2) < 5000, "Tr.bound's range"
        assert c.Cin % 64 == 0 and c.Cout % 64 == 0 and (np.abs(D['bias']) >= 0.5).all()
        live = np.zeros(c.x_rows_total, dtype=bool)
        for n in range(c.N):
            live[n * c.per: n * c.per + c.need] = True
        assert (D['x'][~live] == B.SENTINEL).all() and (~live).sum() == c.N * c.gap + 3 and (np.abs(D['x'][live]) < 10).all()
        for f in c.fused:
            assert f.pad_mode == 0 or (f.pad_l < c.Tout and f.pad_r < c.Tout)
            lens = D['fused'][f.name]['lens']
            assert lens is None or (c.Tout in lens and lens.min() < c.Tout)
    assert A.gap == 4 and A.Tout % 16 != 0 and all(A.Tout % bn for bn in (128, 144, 256))
    assert Bc.stride == 2 and Bc.fused[0].pad_l == 4 and Bc.fused[0].pad_r == 5
    assert Cc.Kw == 1 and Cc.Cout == 64 and Cc.fused[0].act == 0 and Cc.fused[0].pad_l + Cc.fused[0].pad_r == 0
    assert Dc.Tout == 19 and Dc.need < 128 and Dc.fused[0].pad_mode == 0 and Dc.fused[0].res
    assert (E.Cin // 64) * E.Kw == 28 and 256 < E.Tout <= 384 and E.Cout == 320
    assert sum(f.out_lo and f.res == 2 for c in CONV_CASES for f in c.fused) == 1
    assert sum(f.acc_in for c in CONV_CASES for f in c.fused) == 1
    assert all(f.tail == 3 for c in CONV_CASES for f in c.fused if f.pad_l + f.pad_r)


def _stats_ratio(good, bad):
    """the GPU test's form both ways: the defect against the good bound, the good value against the defect's bound"""
    r = max(ratio(bad['s1'].v, good['s1'].v, good['s1'].bound()), ratio(bad['s2'].v, good['s2'].v, good['s2'].bound()))
    back = max(ratio(good['s1'].v, bad['s1'].v, bad['s1'].bound()), ratio(good['s2'].v, bad['s2'].v, bad['s2'].bound()))
    return r, back


def _alone(c, y32, defect=None, launches=1):
    depth = R.stats_sum_depth_max(c.N, c.Tout, launches=launches)
    return dict(zip(('s1', 's2'), R.conv_stats_ref(y32, depth, defect=defect)))


@pytest.mark.parametrize('defect', R.STATS_DEFECTS + R.ELEMENT_DEFECTS)
@pytest.mark.parametrize('c', CONV_CASES, ids=lambda c: c.name)
def test_plain_defects_exceed_the_bound_where_they_apply(c, defect):
    """proved here, without a GPU: a kernel with this defect cannot pass a GPU case the defect can show on"""
    D = R.make_conv_case(c)
    for acc_in in (False, True):
        good, bad = R.conv_ref_of(c, D, acc_in=acc_in), R.conv_ref_of(c, D, defect=defect, acc_in=acc_in)
        applies = R.conv_defect_applies(c, defect, acc_in=acc_in)
        if defect == 'stats_of_rounded_y':
            # the epilogue-alone bound only (conv_defect_applies): the fp32 value of the store stands in for the device's
            y32 = good['v'].v.astype(np.float32)
            r, back = _stats_ratio(_alone(c, y32), _alone(c, y32, defect))
            assert r > 250 and back > 250, (c.name, r, back)
            full, _ = _stats_ratio(good, bad)
            print(f'{c.name} {defect}: epilogue alone {r:.0f}x, full bound {full:.2f}x')
            assert full < 1 or c.name[0] not in 'BDE', (c.name, full, 'B, D and E hide it inside the full bound: why it is not used')
        elif defect in R.ELEMENT_DEFECTS:
            r = ratio(bad['v'].v, good['v'].v, good['v'].bound())
            back = ratio(good['v'].v, bad['v'].v, bad['v'].bound())
            if applies:
                print(f'{c.name} {defect}: {r:.1f}x the per-element bound')
                assert r > 1 and back > 1, (c.name, defect, r, back)
                assert defect != 'one_product_dropped' or r >= 10, r
            else:
                assert np.array_equal(bad['v'].v, good['v'].v), (c.name, defect, 'the defect has nothing to act on here')
        else:
            r, back = _stats_ratio(good, bad)
            if applies:
                print(f'{c.name} {defect} acc_in={acc_in}: {r:.1f}x the full bound')
                assert r > 1 and back > 1, (c.name, defect, acc_in, r, back)
                if defect == 'last_row_dropped':
                    r1 = ratio(bad['s1'].v, good['s1'].v, good['s1'].bound())
                    assert r1 > 1, (c.name, 's1 alone shows a dropped row', r1)
                    est = R.dropped_row_over_full_bound(c)
                    print(f'{c.name} a dropped row over the full bound of s1: {r1:.2f} measured, {est:.2f} estimated')
                    assert acc_in or 0.5 < r1 / est < 2, (c.name, r1, est, 'the predicate is the ratio it stands for')
            elif defect == 'last_row_dropped':              # too many rows for the full bound: the epilogue-alone bound shows it
                y32 = good['v'].v.astype(np.float32)
                r, back = _stats_ratio(_alone(c, y32), _alone(c, y32, defect))
                assert r > 1 and back > 1, (c.name, defect, r, back)
            else:
                assert np.array_equal(bad['s1'].v, good['s1'].v) and np.array_equal(bad['s2'].v, good['s2'].v), (c.name, defect)


@pytest.mark.parametrize('defect', R.FUSED_DEFECTS)
@pytest.mark.parametrize('c,f', VARIANTS, ids=lambda v: v.name)
def test_fused_defects_exceed_the_bound_where_they_apply(c, f, defect):
    """the epilogue's own four (a dropped product or a misplaced utterance is pinned on the plain fp32 store, where no bf16
    rounding, clamp or mask stands between the accumulator and the check)"""
    D = R.make_conv_case(c)
    good, bad = R.fused_ref_of(c, D, f)['a'], R.fused_ref_of(c, D, f, defect=defect)['a']
    r_out = R_SPLIT if f.out_lo else R_BF16
    rows = f.pad_l + c.Tout + f.pad_r
    g, b = good.v[:, :rows], bad.v[:, :rows]
    if R.conv_defect_applies(c, defect, f=f):
        r, back = ratio(b, g, good.bound(r_out)[:, :rows]), ratio(g, b, bad.bound(r_out)[:, :rows])
        print(f'{c.name} {f.name} {defect}: {r:.1f}x the per-element bound')
        assert r > 1 and back > 1, (c.name, f.name, defect, r, back)
    else:
        assert np.array_equal(b, g), (c.name, f.name, defect, 'the defect has nothing to act on here')


def test_a_dropped_row_of_3900_shows_against_the_epilogue_alone_bound_only():
    """case F (stream-K): inside the full bound, so conv_defect_applies leaves it to the epilogue-alone bound -- which shows it"""
    c = R.CONV_SK
    D = R.make_conv_case(c)
    good = R.conv_ref_of(c, D)
    full, _ = _stats_ratio(good, R.conv_ref_of(c, D, defect='last_row_dropped', v=good['v']))
    y32 = good['v'].v.astype(np.float32)
    for defect in ('last_row_dropped', 'stats_of_rounded_y'):
        r, back = _stats_ratio(_alone(c, y32), _alone(c, y32, defect))
        print(f'{c.name} {defect}: epilogue alone {r:.0f}x; a dropped row against the full bound {full:.2f}x')
        assert r > 100 and back > 100, (defect, r, back)
    est = R.dropped_row_over_full_bound(c)
    assert full < 1 and est < 1 and 0.5 < full / est < 2, (full, est)
    assert not R.conv_defect_applies(c, 'last_row_dropped') and R.conv_defect_applies(R.CONV_E, 'last_row_dropped')


def test_one_case_shows_every_defect():
    """case A, with its two fused variants and its accumulate launch: every defect applies to it (and the tests above prove that
    where a defect applies it lies outside the bound)"""
    A = R.CONV_A
    for d in R.CONV_DEFECTS:
        assert any(R.conv_defect_applies(A, d, acc_in=a, f=f) for a in (False, True) for f in (None,) + A.fused), d


def test_split_and_stream_k_floors_of_case_e():
    """the GPU sweep over case E counts launches that really split (w2l_conv_plan out[2] > 1) or really ran stream-K (out[3] > 0)
    and asserts floors; the floors are what the geometry yields with the host-only plan query, here"""
    from wav2letter_pytorch_amd import _lib as L
    c = R.CONV_E
    ws = L.lib.w2l_conv_splitk_workspace_bytes(c.N, c.Cout, c.Tout)
    out = (ctypes.c_int * 8)()
    split = sk = 0
    for idx in range(2 * R.NSHAPES, 16 * R.NSHAPES, 5):
        if L.lib.w2l_conv_plan(c.N, c.Cin, c.Cout, c.Tout, c.Kw, c.stride, c.dil, 2, ws, idx, out) == 0:
            split += out[2] > 1
            sk += out[3] > 0
    assert (split, sk) == (R.E_SPLIT_FLOOR, R.E_STREAMK_FLOOR), (split, sk)
    # case F: E's geometry at the smallest batch where stream-K really runs on several shapes
    c = R.CONV_SK
    assert (c.Cin, c.Cout, c.Kw, c.stride, c.dil, c.Tout) == (R.CONV_E.Cin, R.CONV_E.Cout, R.CONV_E.Kw, 1, 1, R.CONV_E.Tout)
    ws = L.lib.w2l_conv_splitk_workspace_bytes(c.N, c.Cout, c.Tout)
    sk = 0
    for idx in range(14 * R.NSHAPES, 16 * R.NSHAPES):
        for flag in (2, 1):
            if L.lib.w2l_conv_plan(c.N, c.Cin, c.Cout, c.Tout, c.Kw, c.stride, c.dil, flag, ws, idx, out) == 0:
                sk += out[3] > 0
    assert sk == R.SK_FLOOR, sk
