"""The three e4m3 kernels -- w2l_conv1d_wgrad_fp8 (csrc/conv_wgrad_fp8.hip), w2l_conv1d_igemm_fp8 and w2l_conv1d_igemm_bnact_fp8
(conv_igemm_kernel<..., F8>) -- called through the C ABI into guarded, NaN-prefilled buffers, against tests/fp8_refs.py (float64;
pinned by tests/test_cpu_fp8_refs.py, which also proves the planted defects and the exactness arithmetic).

Two operand families (fp8_refs' docstring).  On the EXACT family (small integers, power-of-two factors) nothing rounds in any
summation order, so the device result must have the reference's fp32 bits: a mismatch is an indexing defect.  On the FULL-RANGE
family (all 254 finite codes, factors that are no powers of two) |got - v| <= (F8_DOT_MARGIN K + c) u A per element; the worst
error / bound is printed per family (direct_helpers.record) at the margin in force and, as "..., margin 1", against (K + c) u A:
the figure F8_DOT_MARGIN = 32 was chosen from (worst 14.56: fp8_refs.F8_DOT_MARGIN).  The device must lie outside the bound of
every planted defect that the float64 reference itself separates from the right result on that case.

A. weight gradient: plans are forced through the tune file ("wgradf8 N Cin Cout Tout Kw splits order" lines, loaded before every
   plan): every split count 1 .. min(16, N tsteps), both block orders, accumulate 0 / 1, descale_dev null / non-null.  Every byte
   behind the rows the contract lets the kernel read is the e4m3 NaN code, so an unclamped read turns dw NaN; with one split and no
   accumulate dw starts as NaN and every element must be written.  The tune cache is process-wide: the keys of these cases are
   used by no other test, and they keep the last plan loaded here.
B. convolution: all 15 block shapes forced, without and with statistics rows; a refused launch must be one the feasibility table
   (pinned to w2l_conv_plan_fp8 on the CPU) refuses and must have written nothing.  fp32 store, bf16 store = bf16_rne of it,
   statistics tile rows (s1 bit-exact per row on the exact family), the data gradient's form (flipped taps, no bias, bf16).
C. fused inference epilogue on the exact family: the accumulator is exact, the whole error is the epilogue's."""
import ctypes
import functools
import os
import tempfile

import numpy as np
import pytest
import torch

import conv_refs as C
import fp8_refs as R
from bn_refs import lens_limits
from direct_helpers import Buf, guards, last_error, ratio, record
from fp8_refs import CONV8_CASES, E4M3, F8_FUSED, F8_PLAIN, F8_STATS, FAMILIES, FUSED8_CASES, NAN8, NF8, WGRAD8_CASES, bf16_rne

pytestmark = pytest.mark.gpu

NAN_ROWS = 384            # allocated NaN-code rows behind x and dy: more than any window reaches past the last row it may read


@pytest.fixture(scope='module')
def L():
    from wav2letter_pytorch_amd import _lib
    assert torch.cuda.is_available()
    _lib.lib.w2l_conv_stats_mode(0)
    return _lib


def wait(what):
    """a HIP error ends the session: nothing more is launched on a device that has faulted"""
    try:
        torch.cuda.synchronize()
    except Exception as e:                              # noqa: BLE001
        pytest.exit(f'HIP error in {what}, nothing more is run: {e}', returncode=3)


def up(a, dtype=torch.float32):
    return None if a is None else Buf(a.shape, dtype, torch.from_numpy(np.ascontiguousarray(a)))


def addr(b):
    return None if b is None else b.t.data_ptr()


def bytes_behind(a, rows):
    """uint8 Buf: `a` followed by `rows` rows of the e4m3 NaN code"""
    b = Buf((a.shape[0] + rows, a.shape[1]), torch.uint8)
    b.t.fill_(NAN8)
    b.t[:a.shape[0]].copy_(torch.from_numpy(a))
    return b


def bits32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_codes(got, want):
    """e4m3 codes equal, the sign of a zero aside"""
    return ((got == want) | (((got & 0x7F) == 0) & ((want & 0x7F) == 0)))


# ================================================================================================================================
# A. the weight gradient
# ================================================================================================================================

class WSetup:
    def __init__(self, c, fam):
        self.c, self.fam = c, fam
        self.D = D = R.make_wgrad8_case(c, fam)
        self.x = bytes_behind(D['x'], NAN_ROWS)
        self.dy = bytes_behind(D['dy'], NAN_ROWS)
        self.dy_ptr = ctypes.c_void_p(self.dy.t.data_ptr() + c.hb * c.Cout)
        self.dd = up(np.array([R.FACTORS[fam][1]], dtype=np.float32))
        self.S, self.A = R.wgrad8_sums(c, D)
        self.bad = {}

    def untouched(self):
        c = self.c
        return bool((self.x.t[c.x_rows_total:] == NAN8).all() and (self.dy.t[c.dy_rows:] == NAN8).all()) and guards(self.x, self.dy, self.dd)

    def good(self, splits, acc, dev):
        return R.wgrad8_finish(self.c, self.D, self.S, self.A, splits, acc, dev)

    def defects(self, splits, acc, dev):
        """name -> (v, bound) of every defect that applies to this launch"""
        out = {}
        for name in R.WGRAD8_DEFECTS:
            if not R.wgrad8_defect_applies(self.c, name, splits, acc, dev):
                continue
            key = (name, splits) if name == 'split_last_step_dropped' else name
            if key not in self.bad:
                index = name not in ('accumulate_ignored_under_atomics', 'descale_dev_ignored')
                self.bad[key] = R.wgrad8_sums(self.c, self.D, defect=name, splits=splits) if index else (self.S, self.A)
            out[name] = R.wgrad8_finish(self.c, self.D, *self.bad[key], splits, acc, dev, defect=name)
        return out


@functools.lru_cache(maxsize=None)
def wsetup(c, fam):
    return WSetup(c, fam)


def load_plan(L, c, splits, order, folder):
    path = os.path.join(folder, f'{c.name}_{splits}_{order}.tune')
    with open(path, 'w') as f:
        f.write(R.TUNE_HEADER + R.tune_line(c, splits, order))
    assert L.lib.w2l_tune_load(path.encode()) == 1, (c.name, splits, order, last_error(L))
    assert L.lib.w2l_wgrad_fp8_needs_zero(*c.key) == int(splits > 1), (c.name, splits, 'needs_zero is splits > 1')


def wgrad8(L, S, dw, acc, dev, **over):
    c = S.c
    a = dict(dy_bstride=c.dy_per * c.Cout, x_bstride=c.per * c.Cin, x_rows_total=c.x_rows_total)
    a.update(over)
    rc = L.lib.w2l_conv1d_wgrad_fp8(S.dy_ptr, a['dy_bstride'], L.ptr(S.x.t), a['x_bstride'], a['x_rows_total'], L.ptr(dw.t), c.N, c.Cin,
                                    c.Cout, c.T, c.Kw, c.dil, R.FACTORS[S.fam][0], L.ptr(S.dd.t) if dev else None, int(acc), L.stream_ptr())
    wait('an e4m3 weight-gradient launch')
    return rc


def check_wgrad8(L, S, splits, order, acc, dev):
    """one launch under the loaded plan"""
    c = S.c
    tag = f'{c.name} {S.fam} splits {splits} order {order} acc {int(acc)} dev {int(dev)}'
    dw = Buf((c.Kw, c.Cout, c.Cin), torch.float32, S.D['dw0'] if acc else None)     # NaN unless accumulate
    if splits > 1 and not acc:
        dw.t.zero_()
    assert wgrad8(L, S, dw, acc, dev) == 0, (tag, last_error(L))
    assert guards(dw) and S.untouched(), (tag, 'a guard, or a byte behind x / dy')
    got = dw.np()
    assert not np.isnan(got).any(), (tag, 'NaN in dw: an unclamped read (NaN code x 0), or an element nobody stored')
    v, b = S.good(splits, acc, dev)
    bad = S.defects(splits, acc, dev)
    if S.fam == 'exact':
        assert np.array_equal(bits32(got), bits32(v)), (tag, 'bits differ on exact operands: an indexing defect',
                                                          np.argwhere(bits32(got) != bits32(v))[:4].tolist())
        for name, (bv, _) in bad.items():
            assert not np.array_equal(bits32(got), bits32(bv)), (tag, name, 'the device agrees with a planted defect')
        return 0.0
    fam = 'wgrad8 full range' + (' atomic' if splits > 1 else '') + (' accumulate' if acc else '')
    record(fam + ', margin 1', tag, ratio(got, v, R.wgrad8_finish(c, S.D, S.S, S.A, splits, acc, dev, margin=1.0)[1]))
    r = record(fam, tag, ratio(got, v, b))
    assert r <= 1, (tag, 'outside (F8_DOT_MARGIN K + c) u A', r)
    for name, (bv, bb) in bad.items():
        if ratio(bv, v, b) > 1:                       # the reference itself separates this defect from the right result here
            assert ratio(got, bv, bb) > 1, (tag, name, 'the device agrees with a planted defect')
    return r


@pytest.mark.parametrize('c', WGRAD8_CASES, ids=lambda c: c.name)
def test_wgrad8_every_plan_against_float64(L, c):
    """every split count 1 .. min(16, N tsteps) x both block orders x accumulate x descale_dev x both families"""
    launches = 0
    with tempfile.TemporaryDirectory() as folder:
        for splits, order in R.wgrad8_plans(c):
            load_plan(L, c, splits, order, folder)
            for fam in FAMILIES:
                S = wsetup(c, fam)
                for acc in (False, True):
                    for dev in (False, True):
                        check_wgrad8(L, S, splits, order, acc, dev)
                        launches += 1
    assert launches == 16 * c.max_splits


def test_wgrad8_argument_checks(L):
    """a dy stride shorter than the rows the K loop walks is refused with a message and nothing is launched; exactly that many
    rows run and are right (case W5: 75 frames, one 128-frame step, dy_per = 128)"""
    c = R.W5
    S = wsetup(c, 'exact')
    assert c.dy_per == c.tsteps * 128
    with tempfile.TemporaryDirectory() as folder:
        load_plan(L, c, 1, 1, folder)
        for short in ((c.tsteps * 128 - 1) * c.Cout, c.T * c.Cout):
            dw = Buf((c.Kw, c.Cout, c.Cin))
            assert wgrad8(L, S, dw, False, True, dy_bstride=short) != 0 and 'dy_bstride holds' in last_error(L), last_error(L)
            assert torch.isnan(dw.t).all() and guards(dw) and S.untouched(), 'something was launched'
        check_wgrad8(L, S, 1, 1, False, True)
        load_plan(L, c, 2, 0, folder)
        dw = Buf((c.Kw, c.Cout, c.Cin))
        assert wgrad8(L, S, dw, False, True, dy_bstride=(c.tsteps * 128 - 1) * c.Cout) != 0 and 'dy_bstride holds' in last_error(L)
        assert torch.isnan(dw.t).all(), 'something was launched'
        # the other refusals of the launcher, each with its message
        for over, says in ((dict(x_bstride=c.per * c.Cin + 8), 'whole rows'), (dict(dy_bstride=c.dy_per * c.Cout + 8), 'whole rows')):
            assert wgrad8(L, S, dw, False, True, **over) != 0 and says in last_error(L), last_error(L)
            assert torch.isnan(dw.t).all(), 'something was launched'


# ================================================================================================================================
# B. the convolution
# ================================================================================================================================

class CSetup:
    def __init__(self, c, fam):
        self.c, self.fam = c, fam
        self.D = D = R.make_conv8_case(c, fam)
        self.x = bytes_behind(D['x'], 64)
        self.w = {False: up(R.w_device8(D), torch.uint8), True: up(R.w_device8(D, True), torch.uint8)}
        self.bias = up(D['bias'])
        self.dd = up(np.array([R.FACTORS[fam][1]], dtype=np.float32))
        self.refs = {}

    def ref(self, flipped, bias, dev, defect=None):
        key = (flipped, bias, dev, defect)
        if key not in self.refs:
            self.refs[key] = R.conv8_ref(self.c, self.D, flipped, bias, dev, defect=defect)
        return self.refs[key]

    def inputs(self):
        return [self.x, self.w[False], self.w[True], self.bias, self.dd]

    def untouched(self):
        return bool((self.x.t[self.c.x_rows_total:] == NAN8).all()) and guards(*self.inputs())

    def partial(self):
        """one NaN row per 128-column tile, then 2 more"""
        rows = self.c.N * -(-self.c.Tout // 128)
        return Buf((rows + 2, 2, self.c.Cout)), rows


@functools.lru_cache(maxsize=None)
def csetup(c, fam):
    return CSetup(c, fam)


def conv8(L, S, k, y_f32, pb=None, dev=True, flipped=False, bias=True):
    c = S.c
    y = Buf((c.N, c.Tout, c.Cout), torch.float32 if y_f32 else torch.bfloat16)
    L.lib.w2l_conv_force_fp8_config(k)
    try:
        rc = L.lib.w2l_conv1d_igemm_fp8(L.ptr(S.x.t), c.per * c.Cin, c.x_rows_total, L.ptr(S.w[flipped].t), L.ptr(y.t), y_f32,
                                        R.FACTORS[S.fam][0], L.ptr(S.dd.t) if dev else None, L.ptr(S.bias.t) if bias else None,
                                        None if pb is None else L.ptr(pb.t), c.N, c.Cin, c.Cout, c.Tout, c.Kw, c.dil, L.stream_ptr())
    finally:
        L.lib.w2l_conv_force_fp8_config(-1)
    wait('an e4m3 implicit GEMM launch')
    return rc, y


def held_y(S, yh, ref, tag, family):
    """the fp32 store against float64: bits on the exact family, the bound on the full-range one"""
    assert not np.isnan(yh).any(), (tag, 'NaN in y')
    if S.fam == 'exact':
        assert np.array_equal(bits32(yh), bits32(ref.v)), (tag, 'bits differ on exact operands: an indexing defect',
                                                          np.argwhere(bits32(yh) != bits32(ref.v))[:4].tolist())
        return
    record(family + ', margin 1', tag, ratio(yh, ref.v, (S.c.K + ref.c8) * R.U * ref.a))
    r = record(family, tag, ratio(yh, ref.v, R.bound_of(ref)))
    assert r <= 1, (tag, 'outside (F8_DOT_MARGIN Kw Cin + c) u A', r)


def outside(S, got, good, bad, tag, name):
    """the device does not agree with a planted defect (full range: where the reference itself separates it from the right result)"""
    if S.fam == 'exact':
        assert not np.array_equal(bits32(got), bits32(bad.v)), (tag, name, 'the device agrees with a planted defect')
    elif ratio(bad.v, good.v, R.bound_of(good)) > 1:
        assert ratio(got, bad.v, R.bound_of(bad)) > 1, (tag, name, 'the device agrees with a planted defect')


def check_conv8(L, S, k, flag):
    """one block shape under one statistics flag: the fp32 and the bf16 store (and the statistics rows); False: refused"""
    c = S.c
    dev = flag == F8_STATS                          # the statistics launches carry the device factor, the plain ones do not
    tag = f'{c.name} {S.fam} shape {k} flag {flag}'
    why = R.f8_cannot_run(c, k, flag)
    assert R.F8_CODE[why] == R.F8_FEASIBLE[c.name][flag][k]
    pb, rows = S.partial() if flag == F8_STATS else (None, 0)
    rc, y32 = conv8(L, S, k, 1, pb, dev)
    if rc != 0:
        assert why, (tag, 'refused without a documented reason', last_error(L))
        assert torch.isnan(y32.t).all() and (pb is None or torch.isnan(pb.t).all()) and guards(y32, pb), (tag, 'refused, yet something was written')
        return False
    assert why is None, (tag, 'ran although it is documented not to', why)
    ref = S.ref(False, True, dev)
    yh = y32.np()
    held_y(S, yh, ref, tag, 'conv8 full range fp32 store')
    pb16 = S.partial()[0] if pb is not None else None
    rc, y16 = conv8(L, S, k, 0, pb16, dev)
    assert rc == 0, (tag, last_error(L))
    assert np.array_equal(y16.bits(), bf16_rne(yh)), (tag, 'bf16 store is not the rounded fp32 store')
    assert guards(y32, y16, pb, pb16) and S.untouched(), tag
    for name in C.ELEMENT_DEFECTS + ('descale_dev_ignored',):
        if R.conv8_defect_applies(c, name, dev):
            outside(S, yh, ref, S.ref(False, True, dev, name), tag, name)
    if pb is None:
        return True
    # the statistics: one row per 128-column tile, every other row keeps its NaN; bit-equal between the two stores
    part = pb.np().astype(np.float64)
    assert np.isfinite(part[:rows]).all() and np.isnan(part[rows:]).all(), (tag, 'rows the launch owns / does not own')
    assert torch.equal(pb.t[:rows].view(torch.int32), pb16.t[:rows].view(torch.int32)), (tag, 'tile rows differ with y_f32')
    got = part[:rows].sum(0)
    g1, g2 = R.conv8_stats(c, S.D, ref, k, descale_dev=dev)
    if S.fam == 'exact':
        assert np.array_equal(bits32(part[:rows, 0]), bits32(R.tile_row_sums(c, ref.v))), (tag, 's1 tile rows differ on exact operands')
        assert np.array_equal(got[0], g1.v), (tag, 'column sums of y')
    rs = [ratio(got[0], g1.v, R.bound_of(g1)), ratio(got[1], g2.v, R.bound_of(g2))]
    record(f'conv8 {S.fam} sums', tag, max(rs))
    assert max(rs) <= 1, (tag, 'statistics outside the bound', rs)
    for name in ('last_row_dropped', 'dead_rows_counted', 'bias_not_in_stats'):
        b1, b2 = R.conv8_stats(c, S.D, ref, k, defect=name, descale_dev=dev)
        if S.fam == 'exact':
            assert not np.array_equal(got[0], b1.v), (tag, name, 'the device agrees with a planted defect')
        elif any(ratio(b.v, g.v, R.bound_of(g)) > 1 for b, g in ((b1, g1), (b2, g2))):
            assert ratio(got[0], b1.v, R.bound_of(b1)) > 1 or ratio(got[1], b2.v, R.bound_of(b2)) > 1, \
                (tag, name, 'the device agrees with a planted defect')
    return True


def check_dgrad_form(L, S, k):
    """the data gradient's launch: flipped-tap weights, no bias, the device factor, bf16 output"""
    c = S.c
    tag = f'{c.name} {S.fam} shape {k} data-gradient form'
    rc, y32 = conv8(L, S, k, 1, None, True, flipped=True, bias=False)
    assert rc == 0, (tag, last_error(L))
    ref = S.ref(True, False, True)
    yh = y32.np()
    held_y(S, yh, ref, tag, 'conv8 full range data-gradient form')
    rc, y16 = conv8(L, S, k, 0, None, True, flipped=True, bias=False)
    assert rc == 0 and np.array_equal(y16.bits(), bf16_rne(yh)), (tag, 'bf16 store is not the rounded fp32 store')
    assert guards(y32, y16) and S.untouched(), tag
    if c.Kw > 1:
        outside(S, yh, ref, S.ref(False, False, True), tag, 'taps not flipped')
    outside(S, yh, ref, S.ref(True, False, True, 'descale_dev_ignored'), tag, 'descale_dev_ignored')


@pytest.mark.parametrize('fam', FAMILIES)
@pytest.mark.parametrize('c', CONV8_CASES, ids=lambda c: c.name)
def test_conv8_every_block_shape_against_float64(L, c, fam):
    S = csetup(c, fam)
    ran = {F8_PLAIN: 0, F8_STATS: 0}
    for k in range(NF8):
        for flag in (F8_PLAIN, F8_STATS):
            ran[flag] += check_conv8(L, S, k, flag)
        check_dgrad_form(L, S, k)
    assert ran == {F8_PLAIN: 15, F8_STATS: 9}, ran


def test_conv8_forced_index_out_of_range_is_refused(L):
    S = csetup(R.F2, 'exact')
    for k in (NF8, 99):
        rc, y = conv8(L, S, k, 1)
        assert rc != 0 and torch.isnan(y.t).all() and guards(y), k


# ================================================================================================================================
# C. the fused inference epilogue
# ================================================================================================================================

def fused8(L, S, f, P, ops, bias, q_scale, k, want_hi=True, want_q=True):
    c = S.c
    out_rows = f.pad_l + c.Tout + f.pad_r + f.tail
    hi = Buf((c.N, out_rows, c.Cout), torch.bfloat16) if want_hi else None
    q = Buf((c.N, out_rows, c.Cout), torch.uint8) if want_q else None
    e = L.BnActEpi(scale=addr(ops['scale']), shift=addr(ops['shift']), res=addr(ops['res']), res_lo=None, act=f.act, lens=addr(ops['lens']),
                   out_hi=addr(hi), out_lo=None, out_rows=out_rows, pad_l=f.pad_l, pad_r=f.pad_r, pad_mode=f.pad_mode)
    L.lib.w2l_conv_force_fp8_config(k)
    try:
        rc = L.lib.w2l_conv1d_igemm_bnact_fp8(L.ptr(S.x.t), c.per * c.Cin, c.x_rows_total, L.ptr(S.w[False].t), R.FUSED8_DESCALE,
                                              L.ptr(S.bias.t) if bias else None, ctypes.byref(e), None if q is None else L.ptr(q.t), q_scale,
                                              None, c.N, c.Cin, c.Cout, c.Tout, c.Kw, c.dil, L.stream_ptr())
    finally:
        L.lib.w2l_conv_force_fp8_config(-1)
    wait('a fused e4m3 inference launch')
    return rc, hi, q


def check_fused8(L, S, f, P, ops, ref, bad, bias, q_scale, k):
    c = S.c
    tag = f'{c.name} {f.name} shape {k}'
    why = R.f8_cannot_run(c, k, F8_FUSED)
    assert R.F8_CODE[why] == R.F8_FEASIBLE[c.name][F8_FUSED][k]
    rc, hi, q = fused8(L, S, f, P, ops, bias, q_scale, k)
    if rc != 0:
        assert why, (tag, 'refused without a documented reason', last_error(L))
        assert torch.isnan(hi.t).all() and (q.t == 0xA5).all() and guards(hi, q), (tag, 'refused, yet something was written')
        return False
    assert why is None, (tag, 'ran although it is documented not to', why)
    rows = ref['rows']
    assert guards(hi, q, *[b for b in ops.values() if b is not None]) and S.untouched(), tag
    assert torch.isnan(hi.t[:, rows:]).all() and (q.t[:, rows:] == 0xA5).all(), (tag, 'rows beyond the padded extent')
    # the bf16 output: the epilogue's own bound, per element
    a = ref['a']
    got = hi.np().astype(np.float64)[:, :rows]
    r = record('fused8 bf16 output', tag, ratio(got, a.v[:, :rows], a.bound(C.R_BF16)[:, :rows]))
    assert r <= 1, (tag, 'bf16 output outside the epilogue bound', r)
    # the e4m3 output: the bound, and the very code wherever the reference is certain of it
    aq = R.Tr(ref['aq'].v[:, :rows], ref['aq'].a[:, :rows], ref['aq'].d)
    qh = q.np()[:, :rows]
    want = np.clip(aq.v, -448, 448)
    assert np.isfinite(E4M3[qh]).all(), (tag, 'a NaN code in the e4m3 output')
    rq = record('fused8 e4m3 output', tag, ratio(E4M3[qh], want, R.e4m3_bound(aq, q_scale)))
    assert rq <= 1, (tag, 'e4m3 output outside its bound', rq)
    codes, sure = R.e4m3_certain(want, aq.bound())
    assert same_codes(qh, codes)[sure].all(), (tag, 'an e4m3 code differs where the reference is certain', int((~same_codes(qh, codes) & sure).sum()))
    assert sure.mean() > 0.99
    # halo rows: the bytes of the frame they mirror, or zero; masked frames: zero
    hb = hi.bits()
    src = ref['src']
    for rrow in range(rows):
        if src[rrow] < 0:
            assert not hb[:, rrow].any() and not qh[:, rrow].any(), (tag, rrow, 'a zero halo row')
        elif rrow - f.pad_l != src[rrow]:
            assert np.array_equal(hb[:, rrow], hb[:, f.pad_l + src[rrow]]) and np.array_equal(qh[:, rrow], qh[:, f.pad_l + src[rrow]]), \
                (tag, rrow, 'a halo row differs from its frame')
    for n, lim in enumerate(lens_limits(c.N, c.Tout, P['lens'])):
        assert not hb[n, f.pad_l + lim: f.pad_l + c.Tout].any() and not qh[n, f.pad_l + lim: f.pad_l + c.Tout].any(), (tag, n, 'a masked frame')
    # the one-output forms
    rc, _, only_q = fused8(L, S, f, P, ops, bias, q_scale, k, want_hi=False)
    assert rc == 0 and torch.equal(only_q.t, q.t) and guards(only_q), (tag, 'the e4m3-only form differs from the two-output form')
    rc, only_hi, _ = fused8(L, S, f, P, ops, bias, q_scale, k, want_q=False)
    assert rc == 0 and np.array_equal(only_hi.bits()[:, :rows], hb[:, :rows]) and guards(only_hi), (tag, 'the bf16-only form differs')
    assert torch.isnan(only_hi.t[:, rows:]).all()
    for name, b in bad.items():
        assert ratio(got, b.v[:, :rows], b.bound(C.R_BF16)[:, :rows]) > 1, (tag, name, 'the device agrees with a planted defect')
    return True


@pytest.mark.parametrize('c', FUSED8_CASES, ids=lambda c: c.name)
def test_fused8_every_built_shape_against_float64(L, c):
    S = csetup(c, 'exact')
    for f, bias, q_scale in R.fused8_variants(c):
        P = R.make_fused8_params(c, f)
        ops = dict(scale=up(P['scale']), shift=up(P['shift']), res=up(P['res'], torch.bfloat16), lens=up(P['lens'], torch.int32))
        v = R.fused8_acc(c, S.D, bias)
        ref = R.fused8_ref(c, f, P, v, q_scale)
        bad = {d: R.fused8_ref(c, f, P, v, q_scale, defect=d)['a'] for d in C.FUSED_DEFECTS if C.conv_defect_applies(c, d, f=f)}
        ran = sum(check_fused8(L, S, f, P, ops, ref, bad, bias, q_scale, k) for k in range(NF8))
        assert ran == 11, (f.name, ran)
