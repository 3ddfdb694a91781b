"""The float64 reference of the dense weight gradient (tests/wgrad_refs.py, used by tests/test_gpu_wgrad_direct.py) pinned on the
CPU: against torch autograd of F.conv1d in float64; every planted defect (wgrad_refs.WGRAD_DEFECTS) shown to lie outside the
bound the GPU test applies (WGRAD_DOT_MARGIN included) on every case whose geometry lets it act, and to change nothing where it
cannot; the operand layout (zero / SENTINEL rows) as the GPU test relies on it; and the sweep table WGRAD_PATHS pinned to
w2l_wgrad_launch_plan, the host-only query that runs the very plan() every launch goes through."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import wgrad_refs as R
from bn_refs import SENTINEL
from direct_helpers import ratio
from wgrad_refs import WGRAD_A, WGRAD_CASES, WGRAD_DEFECTS

ALL_CASES = WGRAD_CASES + [R.group_case(i, d) for d in R.GROUP_DILS for i in range(len(R.GROUP_LAYERS))]


def rel(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def t64(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))


def autograd_dw(c, D):
    """[Kw][Cout][Cin] float64: the weight gradient of F.conv1d on the rows each utterance needs, by autograd"""
    x = t64(R.x_view(c, D)[:, :c.need]).transpose(1, 2)
    w = torch.zeros(c.Cout, c.Cin, c.Kw, dtype=torch.float64, requires_grad=True)
    y = F.conv1d(x, w, None, stride=c.stride, dilation=c.dil)
    assert y.shape == (c.N, c.Cout, c.Tout)
    y.backward(t64(R.dy_view(c, D)[:, :c.Tout]).transpose(1, 2))
    return w.grad.permute(2, 0, 1).numpy()


@pytest.mark.parametrize('c', ALL_CASES, ids=lambda c: c.name)
def test_wgrad_ref_matches_torch_float64_autograd(c):
    D = R.make_wgrad_case(c)
    want = autograd_dw(c, D)
    for dw0 in (False, True):
        ref = R.wgrad_ref_of(c, D, dw0=dw0)
        full = want + D['dw0'].astype(np.float64) if dw0 else want
        assert ref.v.shape == (c.Kw, c.Cout, c.Cin) and rel(ref.v, full) <= 1e-12
        assert ref.d == c.K + dw0 and ref.d + 2 <= 523 and (ref.a >= np.abs(ref.v) * (1 - 1e-15)).all()
    assert c.K <= 520


@pytest.mark.parametrize('c', ALL_CASES, ids=lambda c: c.name)
def test_operand_layout(c):
    """what the GPU test relies on: the x buffer ends exactly at the last row a live product reads (but for the gap rows of a
    case that has them), dy holds zeros in rows [Tout, roundup64(Tout)) and SENTINEL in every row no 64-row step covers, every
    value is a finite bf16 value, the SENTINEL too"""
    D = R.make_wgrad_case(c)
    x, dy = D['x'], D['dy']
    sent = float(R.bf16(np.full(1, SENTINEL))[0])
    assert np.isfinite(sent) and sent > 1000
    assert np.array_equal(R.bf16(x), x) and np.array_equal(R.bf16(dy), dy) and np.isfinite(x).all() and np.isfinite(dy).all()
    assert x.shape == (c.x_rows_total, c.Cin) and c.x_rows_total == (c.N - 1) * c.per + c.need + c.gap
    xv = R.x_view(c, D)
    assert (np.abs(xv[:, :c.need]) < 100).all() and (xv[:, c.need:] == sent).all()
    r64 = R.roundup64(c.Tout)
    assert c.dy_per >= r64 and c.dy_per - c.Tout >= c.hb and dy.shape[0] == c.hb + c.N * c.dy_per
    dv = R.dy_view(c, D)
    assert (dy[:c.hb] == sent).all() and (np.abs(dv[:, :c.Tout]) < 100).all()
    assert not dv[:, c.Tout:r64].any() and (dv[:, r64:] == sent).all()


def test_the_cases_reach_what_they_are_there_for():
    A, B, C_, D_, E, F_ = WGRAD_CASES
    assert A.Tout % 64 == 1 and B.Tout % 64 == 63 and D_.Tout % 64 == 0 and A.gap == 4 and all(c.gap == 0 for c in WGRAD_CASES[1:])
    assert A.Cin % 128 == 64 and A.Cout % 128 == 64 and B.Cin == 64 and C_.Cout % 128 == 64 and D_.Cout == 64
    assert (A.Kw % 2, A.Kw % 3, A.Kw % 4, A.Kw % 6) == (1, 1, 3, 1)             # last group of 1; one-tap second group; idle second group
    assert B.Kw % 3 == 2 and B.dil == 4 and E.dil == 5 and C_.stride == 2 and D_.Kw == 1 and E.N == 1
    assert [c.steps for c in WGRAD_CASES] == [6, 4, 4, 5, 4, 12]
    assert 4 <= R.tiles2(F_) <= 8 and R.tiles2(F_) * F_.steps == 48


@pytest.mark.parametrize('c', WGRAD_CASES, ids=lambda c: c.name)
def test_every_defect_lies_outside_the_bound(c):
    D = R.make_wgrad_case(c)
    shown = 0
    for dw0 in (False, True):
        good = R.wgrad_ref_of(c, D, dw0=dw0)
        for name in WGRAD_DEFECTS:
            bad = R.wgrad_ref_of(c, D, dw0=dw0, defect=name)
            if R.wgrad_defect_applies(c, name, dw0=dw0):
                # the defective result is outside the good bound, and the good result outside the defective one's (the form the
                # GPU test asserts: the device must not agree with the defect)
                assert ratio(bad.v, good.v, R.margin(good)) > 1, (c.name, name, dw0)
                assert ratio(good.v, bad.v, R.margin(bad)) > 1, (c.name, name, dw0)
                shown += not dw0
            else:
                assert np.array_equal(bad.v, good.v), (c.name, name, dw0, 'acts where it is said not to')
    if c is WGRAD_A:
        assert shown >= 5, shown
    # a result that is right stays inside: the fp32 rounding of the exact value, and a sequential fp32 sum of one element
    good = R.wgrad_ref_of(c, D)
    assert ratio(good.v.astype(np.float32), good.v, R.margin(good)) <= 1
    dyv, xv = R.dy_view(c, D), R.x_view(c, D)
    acc = np.float32(0)
    for n in range(c.N):
        for t in range(c.Tout):
            acc = np.float32(acc + dyv[n, t, -1] * xv[n, t * c.stride + (c.Kw - 1) * c.dil, -1])
    assert abs(float(acc) - good.v[-1, -1, -1]) <= R.margin(good)[-1, -1, -1]


def test_every_defect_applies_somewhere():
    for name in WGRAD_DEFECTS:
        assert any(R.wgrad_defect_applies(c, name, dw0=True) for c in WGRAD_CASES), name
    assert sum(R.wgrad_defect_applies(WGRAD_A, name) for name in WGRAD_DEFECTS) >= 5
    assert 1 <= R.WGRAD_DOT_MARGIN <= 4


# ---- the sweep table -----------------------------------------------------------------------------------------------------------------

@pytest.fixture()
def L():
    from wav2letter_pytorch_amd import _lib
    _lib.lib.w2l_wgrad_force_plan(0, -1)
    _lib.lib.w2l_wgrad_deterministic(0)
    return _lib


def query(L, c, ws, count, order):
    full = max(int(L.lib.w2l_wgrad_workspace_bytes(c.Cin, c.Cout, c.Kw)), int(L.lib.w2l_wgrad_dealt_workspace_bytes(c.Cin, c.Cout, c.Kw)))
    out = (ctypes.c_int * len(R.PLAN_FIELDS))()
    assert L.lib.w2l_wgrad_launch_plan(*c.shape, full if ws else 0, count, order, out) == 0, L.lib.w2l_last_error()
    return dict(zip(R.PLAN_FIELDS, list(out)))


@pytest.mark.parametrize('c', WGRAD_CASES, ids=lambda c: c.name)
def test_sweep_table_is_what_the_launcher_answers(L, c):
    plans = R.wgrad_plans(c)
    assert len(plans) == len(set(plans)) == len(R.WGRAD_PATHS[c.name])
    for p, code in zip(plans, R.WGRAD_PATHS[c.name]):
        r = query(L, c, *p)
        assert r['total_steps'] == c.steps and r['ok'] == 1
        assert R.wgrad_path(r, p[2]) == code, (c.name, p, r)
        # what the code says is what the plan holds
        assert code[0] == 'f' or r['needs_zero'] == int(code[0] in 'akK'), (p, code, r)
        if code[0] == 'd':
            assert r['slabs'] and r['tiles'] <= r['G'] <= r['tiles'] * c.steps and r['grid_x'] == r['G'] + r['dealt_b']
        if code[0] in 'sa':
            assert r['splits'] >= 2 and r['grid_y'] == r['splits']
        if code[1] in '36':
            assert c.stride == 1 and c.dil <= 4 and r['kwblk'] == int(code[1])


def test_every_path_occurs():
    total = {}
    for c in WGRAD_CASES:
        for name, n in R.path_counts(R.WGRAD_PATHS[c.name]).items():
            total[name] = total.get(name, 0) + n
    assert set(total) == set(R.ALL_PATHS), set(R.ALL_PATHS) - set(total)
    assert all(n >= 2 for n in total.values()), total
    per = {c.name: R.path_counts(R.WGRAD_PATHS[c.name]) for c in WGRAD_CASES}
    # what the cases are there for: the stride-2 case and dilation 5 narrow every m32 / three-tap plan, the one-tap layer runs
    # the one-tap kernels, case A has both three-tap forms, case F dealt plans with second segments
    assert 'taps3' not in per['C_stride2'] and 'm32' not in per['C_stride2'] and per['C_stride2']['narrowed'] >= 40
    assert 'taps3' not in per['E_dil5_one_utterance'] and per['E_dil5_one_utterance']['narrowed'] >= 40
    assert per['D_one_tap']['taps1'] + per['D_one_tap']['m32'] == len(R.WGRAD_PATHS['D_one_tap'])
    assert per['A_one_live_row']['taps3'] >= 10 and per['A_one_live_row']['taps6'] >= 10 and per['F_12_steps']['dealt'] == 20


def test_dealt_plans_of_case_f_have_second_segments(L):
    c = R.WGRAD_F
    second = 0
    for p, code in zip(R.wgrad_plans(c), R.WGRAD_PATHS[c.name]):
        if code[0] == 'd':
            second += query(L, c, *p)['dealt_b'] > 0
    assert second >= 10, second
