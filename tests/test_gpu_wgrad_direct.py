"""The dense weight-gradient kernels (csrc/conv_wgrad_kernel.h through conv_wgrad.hip and the three-tap code object of
conv_wgrad3_dev.hip) called through the C ABI into guarded, NaN-prefilled buffers, against tests/wgrad_refs.py (float64; pinned
by tests/test_cpu_wgrad_refs.py, which also proves that every planted defect lies outside the bound used here wherever it can
act, and pins the table of forced plans, WGRAD_PATHS, to the host-only plan query).  Per launch of a forced plan:

  1. |dw - v| <= WGRAD_DOT_MARGIN (N Tout (+ 1) + 2) u A PER ELEMENT, v and A from the float64 reference;
  2. no NaN anywhere in dw: the x buffer ends exactly at the last row a live product reads and sits in a larger allocation whose
     remaining rows are NaN, so a read past x_rows_total that the kernel failed to clamp shows as NaN x 0 = NaN;
  3. the guards of dw, x, dy and of the workspace are intact;  4. the tickets (ws[:65536]) are back at zero;
  5. needs_zero of w2l_wgrad_launch_plan is what w2l_wgrad_needs_zero_x says under the hook;
  6. a launch that needs no zero fill runs over a NaN-filled dw (nothing of it may survive), one that needs it over zeros;
  7. the result lies OUTSIDE the bound of every planted defect that applies to the case:
        one_product_dropped              the largest product of the last element is missing
        last_row_dropped                 row Tout - 1 of the last utterance is missing in the last ci tile
        next_utterance_row               utterance n of x taken from row n * need, not n * per
        tail_row_clamped_early           x_max_row one too small
        edge_channels_shifted            the Cin - 8 / Cout - 8 staging clamp leaking into the last 8 stored channels
        last_tap_from_idle_group         the last tap of a partial tap group takes the tap before it
        accumulate_dropped_in_edge_tile  accumulate = 1 ignored in the last co tile
every dy row the contract does not require to be zero and every x gap row holds a large finite value (SENTINEL).

The path every forced plan takes is the one WGRAD_PATHS records, so the per-path launch counts of a sweep are the table's.
This file forces plans (a thread-local hook) and restores w2l_wgrad_force_plan(0, -1) / w2l_wgrad_deterministic(0) after every
launch.  The tuner test is the last one: what it remembers for case F's shape stays in the library's process-wide table."""
import contextlib
import ctypes
import functools

import numpy as np
import pytest
import torch

import wgrad_refs as R
from direct_helpers import Buf, guards, last_error, ratio, record
from wgrad_refs import WGRAD_A, WGRAD_CASES, WGRAD_DOT_MARGIN, WGRAD_E, WGRAD_F

pytestmark = pytest.mark.gpu

NAN_ROWS = 256            # allocated NaN rows behind x: more than any window reaches past the last needed row (64 s + 6 d + 4)
FAMILY = {'u': 'wgrad plain', 'a': 'wgrad split atomic', 'f': 'wgrad split atomic', 's': 'wgrad slabs', 'k': 'wgrad stream-K',
          'K': 'wgrad stream-K', 'd': 'wgrad dealt'}
FORM_FAMILY = {'m': 'wgrad m32', '3': 'wgrad taps3/6', '6': 'wgrad taps3/6'}


@pytest.fixture(scope='module')
def L():
    from wav2letter_pytorch_amd import _lib
    assert torch.cuda.is_available()
    return _lib


def wait(what):
    """a HIP error ends the session: nothing more is launched on a device that has faulted"""
    try:
        torch.cuda.synchronize()
    except Exception as e:                              # noqa: BLE001
        pytest.exit(f'HIP error in {what}, nothing more is run: {e}', returncode=3)


@contextlib.contextmanager
def forced(L, count, order):
    L.lib.w2l_wgrad_force_plan(count, order)
    try:
        yield
    finally:
        L.lib.w2l_wgrad_force_plan(0, -1)
        L.lib.w2l_wgrad_deterministic(0)


@functools.lru_cache(maxsize=None)
def refs(c):
    """operands and references of a case, computed once: (v, bound) of the good result and of every applicable defect, without
    and with the accumulate operand"""
    D = R.make_wgrad_case(c)
    out = dict(D=D)
    for dw0 in (False, True):
        good = R.wgrad_ref_of(c, D, dw0=dw0)
        bad = {}
        for name in R.WGRAD_DEFECTS:
            if R.wgrad_defect_applies(c, name, dw0=dw0):
                b = R.wgrad_ref_of(c, D, dw0=dw0, defect=name)
                bad[name] = (b.v, R.margin(b))
        out[dw0] = (good, R.margin(good), bad)
    return out


class Setup:
    """device copies of a case: x with NaN rows behind it, dy, the zero-filled workspace"""

    def __init__(self, L, c, with_ws=True):
        self.c = c
        self.R = refs(c)
        D = self.R['D']
        self.x = Buf((c.x_rows_total + NAN_ROWS, c.Cin), torch.bfloat16)
        self.x.t[:c.x_rows_total].copy_(torch.from_numpy(D['x']))
        self.dy = Buf(D['dy'].shape, torch.bfloat16, torch.from_numpy(D['dy']))
        self.dy_ptr = ctypes.c_void_p(self.dy.t.data_ptr() + c.hb * c.Cout * 2)
        self.ws_bytes = max(int(L.lib.w2l_wgrad_workspace_bytes(c.Cin, c.Cout, c.Kw)), int(L.lib.w2l_wgrad_dealt_workspace_bytes(c.Cin, c.Cout, c.Kw)))
        self.ws = None
        if with_ws:
            self.ws = Buf((self.ws_bytes,), torch.uint8)
            self.ws.t.zero_()

    def untouched(self):
        """the NaN rows behind x are still NaN, every guard is intact, the tickets are back at zero"""
        c = self.c
        return bool(torch.isnan(self.x.t[c.x_rows_total:]).all()) and guards(self.x, self.dy, self.ws) and \
            (self.ws is None or not self.ws.t[:65536].any())

    def new_dw(self, zero=False, init=None):
        c = self.c
        dw = Buf((c.Kw, c.Cout, c.Cin), torch.float32, init)
        if zero:
            dw.t.zero_()
        return dw

    def item(self, L, dw, **over):
        c = self.c
        a = dict(dy_bstride=c.dy_per * c.Cout, x_bstride=c.per * c.Cin, x_rows_total=c.x_rows_total)
        a.update(over)
        return L.WgradItem(self.dy_ptr.value, a['dy_bstride'], self.x.t.data_ptr(), a['x_bstride'], a['x_rows_total'], dw.t.data_ptr(),
                           c.Cin, c.Cout, c.Kw, 0)


def query(L, S, ws, count, order):
    out = (ctypes.c_int * len(R.PLAN_FIELDS))()
    assert L.lib.w2l_wgrad_launch_plan(*S.c.shape, S.ws_bytes if ws else 0, count, order, out) == 0, last_error(L)
    return dict(zip(R.PLAN_FIELDS, list(out)))


def launch(L, S, dw, ws, count, order, accumulate=0, **over):
    """one w2l_conv1d_wgrad_ws under the forced plan; returns rc"""
    c = S.c
    a = dict(dy_bstride=c.dy_per * c.Cout, x_bstride=c.per * c.Cin, x_rows_total=c.x_rows_total)
    a.update(over)
    with forced(L, count, order):
        rc = L.lib.w2l_conv1d_wgrad_ws(S.dy_ptr, a['dy_bstride'], L.ptr(S.x.t), a['x_bstride'], a['x_rows_total'], L.ptr(dw.t), *c.shape,
                                       accumulate, L.ptr(S.ws.t) if ws else None, S.ws_bytes if ws else 0, L.stream_ptr())
    wait('a weight-gradient launch')
    return rc


def held(S, got, tag, families, dw0=False):
    """assertions 1, 2 and 7 on a result; records the worst error / bound under every family"""
    good, bound, bad = S.R[dw0]
    assert not np.isnan(got).any(), (tag, 'NaN in dw: an unclamped read of the x window, or an element nobody stored')
    r = ratio(got, good.v, bound)
    for fam in families:
        record(fam, tag, r)
    assert r <= 1, (tag, 'outside WGRAD_DOT_MARGIN (d + 2) u A', r)
    for name, (v, b) in bad.items():
        assert ratio(got, v, b) > 1, (tag, name, 'the device agrees with a planted defect')
    return r


def run_plan(L, S, plan, accumulate=0, dw0=None):
    """assertions 1-7 on one forced plan; returns (path code, dw on the host)"""
    ws, count, order = plan
    c = S.c
    r = query(L, S, ws, count, order)
    code = R.wgrad_path(r, order)
    with forced(L, count, order):
        assert r['needs_zero'] == L.lib.w2l_wgrad_needs_zero_x(*c.shape, S.ws_bytes if ws else 0), (c.name, plan)
    assert r['needs_zero'] == (r['atomic'] if code[0] == 'f' else int(code[0] in 'akK')), (c.name, plan, r)
    dw = S.new_dw(zero=bool(r['needs_zero'])) if dw0 is None else S.new_dw(init=dw0)
    rc = launch(L, S, dw, ws, count, order, accumulate)
    assert rc == 0, (c.name, plan, last_error(L))
    assert guards(dw) and S.untouched(), (c.name, plan, 'a guard, a NaN row behind x or a ticket')
    got = dw.np()
    fams = [FAMILY[code[0]]] + ([FORM_FAMILY[code[1]]] if code[1] in FORM_FAMILY else [])
    if accumulate:
        fams = ['wgrad accumulate']
    held(S, got, f'{c.name} ws {int(ws)} count {count} order {order} {code}', fams, dw0=dw0 is not None)
    return code, got


# ================================================================================================================================

def test_plain_plan_obeys_its_bound(L):
    """the one number that is not derived: the worst error / bound of the unsplit two-tap plan (order 1, count 1) against float64
    over the six cases, with the bound taken at margin 1, must not exceed WGRAD_DOT_MARGIN"""
    worst = 0.0
    for c in WGRAD_CASES:
        S = Setup(L, c, with_ws=False)
        dw = S.new_dw()
        assert query(L, S, False, 1, 1)['needs_zero'] == 0
        assert launch(L, S, dw, False, 1, 1) == 0, last_error(L)
        assert guards(dw) and S.untouched()
        good = S.R[False][0]
        got = dw.np()
        assert not np.isnan(got).any(), c.name
        worst = max(worst, record('wgrad plain, margin 1', c.name, ratio(got, good.v, good.bound())))
    assert worst <= WGRAD_DOT_MARGIN <= 4, worst


@pytest.mark.parametrize('c', WGRAD_CASES, ids=lambda c: c.name)
def test_every_forced_plan_against_float64(L, c):
    """the sweep of wgrad_refs.wgrad_plans: every plan takes the path WGRAD_PATHS records for it (a forced form that silently
    narrows to another kernel counts as what it ran as), so the launches per path are the table's; block order (order bit 0)
    only changes which block gets which tile: on unsplit and slab plans order o and o ^ 1 give bit-identical dw"""
    S = Setup(L, c)
    ran, bits = [], {}
    for plan, code in zip(R.wgrad_plans(c), R.WGRAD_PATHS[c.name]):
        really, got = run_plan(L, S, plan)
        assert really == code, (c.name, plan, really, 'not the path the table records')
        ran.append(really)
        if code[0] in 'us':
            bits[plan] = got.view(np.uint32)
    assert R.path_counts(ran) == R.path_counts(R.WGRAD_PATHS[c.name]) and len(ran) == len(R.wgrad_plans(c))
    pairs = 0
    for (ws, count, order), b in bits.items():
        if not order & 1 and (ws, count, order | 1) in bits:
            assert np.array_equal(b, bits[(ws, count, order | 1)]), (c.name, ws, count, order, 'block order changed the bits')
            pairs += 1
    assert pairs == 25, pairs            # (with a workspace: 4 counts, without: count 1) x five forms


@pytest.mark.parametrize('c', WGRAD_CASES, ids=lambda c: c.name)
def test_accumulate_on_its_three_paths(L, c):
    """accumulate = 1 over a random fp32 dw0: within the bound of wgrad_ref(dw0=...) on every path; where ONE block owns an
    element (unsplit, slabs, dealt) the kernel does *dst += v once, so the result is fp32(dw0 + the accumulate = 0 result of the
    same plan) bit for bit; atomic splits and stream-K pieces add in arrival order"""
    S = Setup(L, c)
    dw0 = S.R['D']['dw0']
    g = R.tiles2(c) + 1
    plans = [(True, 1, 1), (True, 1, 17), (True, 2, 1), (True, c.steps, 21), (True, 3, 9), (True, g, R.DEALT | 1), (True, g, R.DEALT | 20),
             (False, 2, 1), (False, 3, 16), (True, 2, R.ATOMIC_WS | 5), (False, 1, 3), (False, 1, 6)]
    seen = set()
    for plan in plans:
        code, plain = run_plan(L, S, plan)
        code2, acc = run_plan(L, S, plan, accumulate=1, dw0=dw0)
        assert code == code2
        seen.add(code[0])
        if code[0] in 'usd':
            assert np.array_equal(acc.view(np.uint32), (dw0 + plain).astype(np.float32).view(np.uint32)), (c.name, plan, code)
    assert seen >= {'u', 's', 'a', 'd'} and seen & {'k', 'K'}, seen


@pytest.mark.parametrize('dil', R.GROUP_DILS)
def test_group_launch_against_float64(L, dil):
    """w2l_conv1d_wgrad_group on four layers: every block form, selections of one, two and four layers in two orders; every
    selected layer within its own per-element bound, layers not selected keep their NaN"""
    layers = [Setup(L, R.group_case(i, dil), with_ws=False) for i in range(len(R.GROUP_LAYERS))]
    launches = 0
    for form in R.FORMS:
        for sel in R.GROUP_SELECTIONS:
            dws = [S.new_dw() for S in layers]
            arr = (L.WgradItem * len(sel))(*[layers[i].item(L, dws[i]) for i in sel])
            rc = L.lib.w2l_conv1d_wgrad_group(arr, len(sel), R.GROUP_N, R.GROUP_TOUT, dil, form, L.stream_ptr())
            wait('a group launch')
            assert rc == 0, (form, sel, last_error(L))
            launches += 1
            for i, (S, dw) in enumerate(zip(layers, dws)):
                assert guards(dw) and S.untouched(), (form, sel, i)
                if i in sel:
                    held(S, dw.np(), f'{S.c.name} form {form} selection {sel}', ['wgrad group'])
                else:
                    assert torch.isnan(dw.t).all(), (form, sel, i, 'a layer that was not selected was written')
    assert launches == len(R.FORMS) * len(R.GROUP_SELECTIONS) == 60


def test_argument_checks(L):
    """a buffer short of a live row is refused with a message and nothing is launched (it used to be clamped onto its last row:
    a wrong gradient without a word); the nearest allowed value runs and is right"""
    c = WGRAD_A
    S = Setup(L, c)
    enough = (c.N - 1) * c.per + c.need
    assert enough == c.x_rows_total - c.gap
    for ws in (True, False):
        dw = S.new_dw()
        assert launch(L, S, dw, ws, 1, 1, x_rows_total=enough - 1) != 0 and 'padded input too small' in last_error(L), last_error(L)
        assert torch.isnan(dw.t).all() and guards(dw) and S.untouched(), 'something was launched'
        assert launch(L, S, dw, ws, 1, 1, dy_bstride=(c.Tout - 1) * c.Cout) != 0 and 'dy_bstride holds' in last_error(L), last_error(L)
        assert torch.isnan(dw.t).all() and guards(dw) and S.untouched(), 'something was launched'
    # exactly enough x rows: the clamp now sits on the last row a live product reads, every plan family still within the bound
    for plan in ((True, 1, 1), (True, 2, 17), (True, 1, 21), (False, 3, 9), (False, 1, 7)):
        ws, count, order = plan
        dw = S.new_dw(zero=bool(query(L, S, ws, count, order)['needs_zero']))
        assert launch(L, S, dw, ws, count, order, x_rows_total=enough) == 0, (plan, last_error(L))
        assert guards(dw) and S.untouched()
        held(S, dw.np(), f'{c.name} exactly enough rows {plan}', ['wgrad exactly enough rows'])
    # dy_bstride of exactly Tout rows: one utterance (with more, rows [Tout, roundup64) of one would be the next one's first rows)
    e = WGRAD_E
    Se = Setup(L, e, with_ws=False)
    assert e.N == 1
    dw = Se.new_dw()
    assert launch(L, Se, dw, False, 1, 1, dy_bstride=(e.Tout - 1) * e.Cout) != 0 and 'dy_bstride holds' in last_error(L)
    assert torch.isnan(dw.t).all()
    assert launch(L, Se, dw, False, 1, 1, dy_bstride=e.Tout * e.Cout) == 0, last_error(L)
    held(Se, dw.np(), f'{e.name} dy_bstride of Tout rows', ['wgrad exactly enough rows'])
    # the group launch makes the same checks per layer
    layers = [Setup(L, R.group_case(i, 1), with_ws=False) for i in (0, 1)]
    g1 = layers[1].c
    for over, says in ((dict(x_rows_total=(g1.N - 1) * g1.per + g1.need - 1), 'padded input too small'),
                       (dict(dy_bstride=(g1.Tout - 1) * g1.Cout), 'dy_bstride holds')):
        dws = [S.new_dw() for S in layers]
        arr = (L.WgradItem * 2)(layers[0].item(L, dws[0]), layers[1].item(L, dws[1], **over))
        rc = L.lib.w2l_conv1d_wgrad_group(arr, 2, R.GROUP_N, R.GROUP_TOUT, 1, 1, L.stream_ptr())
        wait('a refused group launch')
        assert rc != 0 and says in last_error(L) and '(layer 1)' in last_error(L), last_error(L)
        assert all(torch.isnan(dw.t).all() and guards(dw) for dw in dws), 'something was launched'
    dws = [S.new_dw() for S in layers]
    arr = (L.WgradItem * 2)(layers[0].item(L, dws[0]), layers[1].item(L, dws[1], x_rows_total=(g1.N - 1) * g1.per + g1.need))
    assert L.lib.w2l_conv1d_wgrad_group(arr, 2, R.GROUP_N, R.GROUP_TOUT, 1, 1, L.stream_ptr()) == 0, last_error(L)
    wait('a group launch')
    for S, dw in zip(layers, dws):
        held(S, dw.np(), f'{S.c.name} group, exactly enough rows', ['wgrad exactly enough rows'])


def test_tuner_then_automatic_launch(L):
    """one w2l_conv1d_wgrad_tune_x on case F, then an automatic launch: within the bound, and w2l_wgrad_launch_plan(0, -1) is the
    query of the remembered plan.  (The choice stays in the library's table under case F's shape: this test is the last one,
    and every other launch of this file pins its count and its form.)"""
    c = WGRAD_F
    S = Setup(L, c)
    scratch = S.new_dw()
    a = (S.dy_ptr, c.dy_per * c.Cout, L.ptr(S.x.t), c.per * c.Cin, c.x_rows_total)
    try:
        rc = L.lib.w2l_conv1d_wgrad_tune_x(*a, L.ptr(scratch.t), *c.shape, 1, L.ptr(S.ws.t), S.ws_bytes, 1, L.stream_ptr())
    finally:
        L.lib.w2l_wgrad_force_plan(0, -1)
        L.lib.w2l_wgrad_deterministic(0)
    wait('the tuner')
    assert rc == 0, last_error(L)
    assert guards(scratch) and S.untouched()
    tuned = L.lib.w2l_wgrad_plan(*c.shape[:5])
    assert tuned >> 8 >= 1
    auto = query(L, S, True, 0, -1)
    assert auto == query(L, S, True, tuned >> 8, tuned & 0xff), (tuned, auto)
    assert auto['needs_zero'] == L.lib.w2l_wgrad_needs_zero_x(*c.shape, S.ws_bytes)
    dw = S.new_dw(zero=bool(auto['needs_zero']))
    assert launch(L, S, dw, True, 0, -1) == 0, last_error(L)
    assert guards(dw) and S.untouched()
    held(S, dw.np(), f'{c.name} tuned plan {tuned >> 8} / {tuned & 0xff}', ['wgrad tuned'])
