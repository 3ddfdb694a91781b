"""conv_igemm_kernel's forward epilogue (EPI = 0: bias, fp32 / bf16 store, accumulate, the BatchNorm partial sums on tile rows or
slot rows) and its fused inference epilogue (EPI = 2: w2l_conv1d_igemm_bnact[_ws]) called through the C ABI into guarded,
NaN-prefilled buffers, against tests/conv_refs.py (float64; pinned by tests/test_cpu_conv_refs.py, which also proves that every
planted defect lies outside the bounds used here wherever it can act).  Per plain launch of a forced configuration:

  1. fp32 store: |y - v| <= (DOT_MARGIN Kw Cin + 1 (+ 1) + 2) u A per element, v and A from the float64 reference;
  2. bf16 store: bit-equal to bf16_rne of the fp32 store of the same configuration (split configurations sum their slabs in
     split order, so for them too);
  3. statistics: the column sums of the partial rows within the FULL bound of conv_stats_ref, and within the EPILOGUE-ALONE bound
     of the sums of that configuration's own fp32 store (depth = conv_refs.stats_sum_depth: the additions the code makes, never
     the row count); tile rows bit-equal between the y_f32 = 0 and 1 launches; rows the launch does not own keep their NaN, slot
     rows beyond the column tiles stay zero; every guard intact; the split-K tickets back at zero;
  4. the device's results lie OUTSIDE the bound of every planted defect that applies (stats_of_rounded_y: the epilogue-alone
     bound only -- the full one hides it; last_row_dropped: the epilogue-alone bound always, the full one up to 600 rows; see
     conv_refs.conv_defect_applies).

A launch that returns an error must do so for one of the reasons below (cannot_run) and must have written nothing -- and a launch
for which none holds must run.  The fused launches are held to the full per-element bound, to the epilogue-alone bound given the
plain fp32 store (acc + bias) of the same configuration, to bit-equal halo rows, zero bits in masked frames and untouched rows
beyond the padded extent.

DOT_MARGIN is the one number not derived: the factor on the dot product's share of the depth, 1 while the matrix unit's
accumulators obey (Kw Cin + 2) u A against float64 (assertion 1 measures exactly that, on every launch).
This file forces configurations and sets the statistics mode; both are thread-local hooks and are reset after every launch."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import conv_refs as R
from conv_refs import CONV_A, CONV_C, CONV_D, CONV_E, CONV_CASES, NSHAPES, R_BF16, R_SPLIT, SHAPES, Tr, bf16_rne
from direct_helpers import Buf, guards, last_error, ratio, record

pytestmark = pytest.mark.gpu

SLOTS = 8
DOT_MARGIN = 1.0
SPILL, LDS_BYTES = 20, 160 * 1024
BASE = 2 * NSHAPES                      # an index is shape + 26 * K-loop structure + 52 * split option (1, 2, 3, 4, 5, 6, 8 blocks,
STREAM_K = 7 * BASE                     # option 7: stream-K)
# one 128-column, one 8-wave 128-column, one 144-, one 256- and one 448-column shape; both K-loop structures
FIVE = (2, 5 + NSHAPES, 7, 12 + NSHAPES, 24)
STRIDE2_MORE = (2 + NSHAPES, 2 + BASE)  # the other stride-2 instantiation (K-loop structure 1) and two blocks per tile of the first
PLAIN, TILE_ROWS, SLOT_ROWS, FUSED = 0, 1, 2, 3          # what a launch carries: the statistics flag of w2l_conv_plan


def cols(idx):
    _, nw, _, ns = SHAPES[idx % NSHAPES]
    return 16 * nw * ns


def cannot_run(c, idx, kind):
    """the documented reasons for which a forced configuration returns an error instead of launching"""
    mw, nw, ms, ns = SHAPES[idx % NSHAPES]
    if idx % NSHAPES == SPILL:
        return 'the spilling shape'
    if c.stride != 1 and idx % NSHAPES != 2:
        return 'stride 2 is built for the 128x128 shape alone'
    xrows = ((cols(idx) - 1) * c.stride + (c.Kw - 1) * c.dil + 1 + 7) & ~7
    if 2 * 16 * mw * ms * 128 + 2 * xrows * 128 > LDS_BYTES:
        return 'LDS'
    if kind == TILE_ROWS and cols(idx) not in (128, 256):
        return 'tile rows need 128 / 256 columns'
    return None


@pytest.fixture(scope='module')
def L():
    from wav2letter_pytorch_amd import _lib
    assert torch.cuda.is_available()
    return _lib


def up(a, dtype=torch.float32):
    return None if a is None else Buf(a.shape, dtype, torch.from_numpy(np.ascontiguousarray(a)))


def addr(b):
    return None if b is None else b.t.data_ptr()


def wait(what):
    """a HIP error ends the session: nothing more is launched on a device that has faulted"""
    try:
        torch.cuda.synchronize()
    except Exception as e:                              # noqa: BLE001
        pytest.exit(f'HIP error in {what}, nothing more is run: {e}', returncode=3)


def redepth(tr, extra, margin_on=0):
    """tr with `extra` more roundings; DOT_MARGIN on `margin_on` of its depth (the dot product's share)"""
    return Tr(tr.v, tr.a, int(round(tr.d + extra + (DOT_MARGIN - 1) * margin_on)))


class Setup:
    """device copies of a case, its references (at chain depth 0: redepth() adds a configuration's), its workspace"""

    def __init__(self, L, c):
        self.c = c
        self.D = D = R.make_conv_case(c)
        self.x, self.x_lo = up(D['x'], torch.bfloat16), None
        self.w, self.w_lo = up(R.w_device(D), torch.bfloat16), None
        self.bias = up(D['bias'])
        self.acc_in = None
        self.ws = torch.zeros(int(L.lib.w2l_conv_splitk_workspace_bytes(c.N, c.Cout, c.Tout)), dtype=torch.uint8, device='cuda')
        self.ref = R.conv_ref_of(c, D, sum_depth=0)
        self.bad = {d: R.conv_ref_of(c, D, defect=d, sum_depth=0, v=self.ref['v']) for d in R.STATS_DEFECTS + R.ELEMENT_DEFECTS
                    if d != 'stats_of_rounded_y' and R.conv_defect_applies(c, d)}
        self.fz = {}
        self.y32 = {}

    def inputs(self):
        return [b for b in (self.x, self.x_lo, self.w, self.w_lo, self.bias, self.acc_in) if b is not None]

    def fused_ops(self, f):
        """device operands and references of a fused variant"""
        if f.name not in self.fz:
            P = self.D['fused'][f.name]
            ops = dict(scale=up(P['scale']), shift=up(P['shift']), res=up(P['res'], torch.bfloat16),
                       res_lo=up(P['res_lo'], torch.bfloat16), lens=up(P['lens'], torch.int32))
            if f.acc_in and self.acc_in is None:
                self.acc_in = up(self.D['acc_in'])
            ref = R.fused_ref_of(self.c, self.D, f)
            bad = {d: R.fused_ref_of(self.c, self.D, f, defect=d)['a'] for d in R.FUSED_DEFECTS
                   if R.conv_defect_applies(self.c, d, f=f)}
            self.fz[f.name] = (ops, ref, bad)
        return self.fz[f.name]

    def partial(self, kind):
        """slot rows: SLOTS zero rows (the kernel adds) then 2 NaN rows; tile rows: one NaN row per 128-column tile then 2 more"""
        c = self.c
        rows = SLOTS if kind == SLOT_ROWS else c.N * -(-c.Tout // 128)
        pb = Buf((rows + 2, 2, c.Cout))
        if kind == SLOT_ROWS:
            pb.t[:rows].zero_()
        return pb, rows


@functools.lru_cache(maxsize=None)
def _setup(L, c):
    return Setup(L, c)


def conv(L, S, idx, y_f32, kind=PLAIN, pb=None, y=None, accumulate=0, x=None, w=None, bias='case', tune_reps=0, **over):
    """one w2l_conv1d_igemm_ws launch (or the tuner) under the forced configuration and the statistics mode; returns (rc, y)"""
    c = S.c
    if y is None:
        y = Buf((c.N, c.Tout, c.Cout), torch.float32 if y_f32 else torch.bfloat16)
    x, w = x or S.x, w or S.w
    b = S.bias if bias == 'case' else bias
    a = dict(x_bstride=c.per * c.Cin, x_rows_total=c.x_rows_total, Cin=c.Cin, Cout=c.Cout, stride=c.stride, y_f32=y_f32)
    a.update(over)
    head = (L.ptr(x.t), a['x_bstride'], a['x_rows_total'], L.ptr(w.t), L.ptr(y.t), a['y_f32'])
    dims = (c.N, a['Cin'], a['Cout'], c.Tout, c.Kw, a['stride'], c.dil)
    tail = (L.ptr(S.ws), S.ws.numel(), L.stream_ptr())
    stats = None if pb is None else L.ptr(pb.t)
    L.lib.w2l_conv_force_tile_config(idx)
    L.lib.w2l_conv_stats_mode(SLOTS if kind == SLOT_ROWS else 0)
    try:
        if tune_reps:
            rc = L.lib.w2l_conv1d_igemm_tune_ws(*head, L.ptr(b.t), stats, *dims, tune_reps, *tail)
        else:
            rc = L.lib.w2l_conv1d_igemm_ws(*head, accumulate, None if b is None else L.ptr(b.t), stats, *dims, *tail)
    finally:
        L.lib.w2l_conv_stats_mode(0)
        L.lib.w2l_conv_force_tile_config(-1)
    wait('an implicit GEMM launch')
    return rc, y


def plan(L, c, kind, idx, ws_bytes):
    """w2l_conv_plan of a forced index: (blocks per tile, stream-K blocks), or None where the launch is refused"""
    out = (ctypes.c_int * 8)()
    if L.lib.w2l_conv_plan(c.N, c.Cin, c.Cout, c.Tout, c.Kw, c.stride, c.dil, kind, ws_bytes, idx, out) != 0:
        return None
    return out[2], out[3]


def same_bits(buf, bits):
    return np.array_equal(buf.bits(), bits)


def unwritten(pb, rows, kind):
    return bool(torch.isnan(pb.t[rows:]).all() and (not pb.t[:rows].any() if kind == SLOT_ROWS else torch.isnan(pb.t[:rows]).all()))


def sums_of(S, pb, rows, idx, kind, launches=1):
    """column sums of the partial rows in float64, after the ownership checks of assertion 3"""
    c = S.c
    part = pb.np().astype(np.float64)
    own = min(rows, c.N * -(-c.Tout // cols(idx)) * launches) if kind == SLOT_ROWS else rows
    assert np.isfinite(part[:own]).all() and np.isnan(part[rows:]).all(), (c.name, idx, 'rows the launch owns / does not own')
    assert kind != SLOT_ROWS or not part[own:rows].any(), (c.name, idx, 'a slot row beyond the column tiles was written')
    return part[:rows].sum(0)


def check_sums(S, got, idx, kind, y32, full, family, tag, launches=1, scale=1):
    """assertion 3 (values) and the statistics half of 4.  full: dict s1, s2 at chain depth 0; y32: this configuration's fp32 store"""
    c = S.c
    depth = R.stats_sum_depth(idx, c.N, c.Tout, SLOTS if kind == SLOT_ROWS else 0, launches)
    out = []
    for k, (name, dot) in enumerate((('s1', c.K), ('s2', 2 * c.K))):
        want = redepth(full[name], depth, dot)
        out.append(ratio(got[k], scale * want.v, scale * want.bound()))
    assert max(out) <= 1, (c.name, idx, tag, 'statistics outside the full bound', out)
    record(family + ' sums, full bound', f'{c.name} idx {idx} {tag}', max(out))
    if y32 is not None:
        alone = R.conv_stats_ref(y32, depth)
        r = max(ratio(got[k], scale * alone[k].v, scale * alone[k].bound()) for k in range(2))
        assert r <= 1, (c.name, idx, tag, 'statistics outside the epilogue-alone bound', r)
        record(family + ' sums, epilogue alone', f'{c.name} idx {idx} {tag}', r)
        for name in ('stats_of_rounded_y', 'last_row_dropped'):             # the two that are held to this bound (conv_defect_applies)
            bad = R.conv_stats_ref(y32, depth, defect=name)
            assert max(ratio(got[k], scale * bad[k].v, scale * bad[k].bound()) for k in range(2)) > 1, \
                (c.name, idx, tag, 'the device agrees with ' + name)


def check_plain(L, S, idx, kind, family):
    """assertions 1-4 on one forced configuration; False: the configuration cannot run this problem (for a documented reason)"""
    c = S.c
    pb, rows = S.partial(kind)
    rc, y32 = conv(L, S, idx, 1, kind, pb)
    why = cannot_run(c, idx, kind)
    if rc != 0:
        assert why, (c.name, idx, kind, 'refused without a documented reason', last_error(L))
        assert torch.isnan(y32.t).all() and unwritten(pb, rows, kind), (idx, 'an error was returned and something was launched')
        return False
    assert why is None, (c.name, idx, kind, 'ran although it is documented not to', why)
    tag = 'slots' if kind == SLOT_ROWS else 'tiles'
    # 1. the fp32 store against float64
    v = S.ref['v']
    yh = y32.np()
    r1 = ratio(yh, v.v, redepth(v, 0, c.K).bound())
    assert r1 <= 1, (c.name, idx, 'fp32 store outside (Kw Cin + 3) u A', r1)
    record(family + ' fp32 store', f'{c.name} idx {idx}', r1)
    # 2. the bf16 store of the same configuration
    pb16, _ = S.partial(kind)
    rc, y16 = conv(L, S, idx, 0, kind, pb16)
    assert rc == 0, (idx, last_error(L))
    assert same_bits(y16, bf16_rne(yh)), (c.name, idx, 'bf16 store is not the rounded fp32 store')
    assert guards(y32, y16, pb, pb16, *S.inputs()), (c.name, idx)
    assert not S.ws[:65536].any(), (idx, 'split-K tickets must be back at zero')
    # 3. the statistics
    got = sums_of(S, pb, rows, idx, kind)
    got16 = sums_of(S, pb16, rows, idx, kind)
    if kind == TILE_ROWS:
        assert torch.equal(pb.t[:rows].view(torch.int32), pb16.t[:rows].view(torch.int32)), (c.name, idx, 'tile rows differ with y_f32')
    check_sums(S, got, idx, kind, yh, S.ref, family, tag)
    check_sums(S, got16, idx, kind, yh, S.ref, family, tag + ' bf16 store')
    # 4. sensitivity
    depth = R.stats_sum_depth(idx, c.N, c.Tout, SLOTS if kind == SLOT_ROWS else 0)
    for name, bad in S.bad.items():
        if name in R.ELEMENT_DEFECTS:
            agrees = ratio(yh, bad['v'].v, redepth(bad['v'], 0, c.K).bound()) <= 1
        else:
            agrees = all(ratio(got[k], redepth(bad[s], depth, dot).v, redepth(bad[s], depth, dot).bound()) <= 1
                         for k, (s, dot) in enumerate((('s1', c.K), ('s2', 2 * c.K))))
        assert not agrees, (c.name, idx, name, 'the device agrees with a planted defect')
    return True


def fused(L, S, f, idx, use_ws=True, **over):
    """one w2l_conv1d_igemm_bnact_ws launch of variant f; returns (rc, out_hi, out_lo)"""
    c = S.c
    ops, _, _ = S.fused_ops(f)
    out_rows = f.pad_l + c.Tout + f.pad_r + f.tail
    epi = over.pop('epi', {})
    alloc = max(out_rows, epi.get('out_rows', 0))       # (an argument check under test never gets a buffer smaller than it claims)
    hi = Buf((c.N, alloc, c.Cout), torch.bfloat16)
    lo = Buf((c.N, alloc, c.Cout), torch.bfloat16) if f.out_lo else None
    e = dict(scale=addr(ops['scale']), shift=addr(ops['shift']), res=addr(ops['res']), res_lo=addr(ops['res_lo']), act=f.act,
             lens=addr(ops['lens']), out_hi=addr(hi), out_lo=addr(lo), out_rows=out_rows, pad_l=f.pad_l, pad_r=f.pad_r,
             pad_mode=f.pad_mode)
    e.update(epi)
    d = L.BnActEpi(**e)
    a = dict(x_bstride=c.per * c.Cin, x_rows_total=c.x_rows_total, Cin=c.Cin, Cout=c.Cout, stride=c.stride)
    a.update(over)
    acc = S.acc_in if f.acc_in else None
    L.lib.w2l_conv_force_tile_config(idx)
    try:
        rc = L.lib.w2l_conv1d_igemm_bnact_ws(L.ptr(S.x.t), a['x_bstride'], a['x_rows_total'], L.ptr(S.w.t), None if acc is None else L.ptr(acc.t),
                                             L.ptr(S.bias.t), ctypes.byref(d), c.N, a['Cin'], a['Cout'], c.Tout, c.Kw, a['stride'], c.dil,
                                             L.ptr(S.ws) if use_ws else None, S.ws.numel() if use_ws else 0, L.stream_ptr())
    finally:
        L.lib.w2l_conv_force_tile_config(-1)
    wait('a fused inference launch')
    return rc, hi, lo


def plain_store(L, S, idx):
    """acc + bias of a configuration: its plain fp32 store, no statistics (the exact input of the epilogue-alone bounds)"""
    if idx not in S.y32:
        rc, y = conv(L, S, idx, 1)
        assert rc == 0, (idx, last_error(L))
        S.y32[idx] = y.np()
    return S.y32[idx]


def check_fused(L, S, f, idx, family):
    c = S.c
    ops, ref, bad = S.fused_ops(f)
    rc, hi, lo = fused(L, S, f, idx)
    why = cannot_run(c, idx, FUSED)
    if rc != 0:
        assert why, (c.name, f.name, idx, 'refused without a documented reason', last_error(L))
        assert torch.isnan(hi.t).all() and (lo is None or torch.isnan(lo.t).all()), (idx, 'an error was returned and something was launched')
        return False
    assert why is None, (c.name, f.name, idx, 'ran although it is documented not to', why)
    assert guards(hi, lo, *S.inputs(), *[b for b in ops.values() if b is not None]), (c.name, f.name, idx)
    assert not S.ws[:65536].any(), (idx, 'split-K tickets must be back at zero')
    rows = f.pad_l + c.Tout + f.pad_r
    tag = f'{c.name} {f.name} idx {idx}'
    assert torch.isnan(hi.t[:, rows:]).all() and (lo is None or torch.isnan(lo.t[:, rows:]).all()), (tag, 'rows beyond the padded extent')
    got = hi.np().astype(np.float64) + (lo.np().astype(np.float64) if lo is not None else 0.0)
    got = got[:, :rows]
    r_out = R_SPLIT if lo is not None else R_BF16
    full = redepth(ref['a'], 0, c.K)
    r = ratio(got, full.v[:, :rows], full.bound(r_out)[:, :rows])
    assert r <= 1, (tag, 'outside the full bound', r)
    record(family + ' full bound', tag, r)
    alone = R.fused_ref_of(c, S.D, f, src=plain_store(L, S, idx))['a']
    ra = ratio(got, alone.v[:, :rows], alone.bound(r_out)[:, :rows])
    assert ra <= 1, (tag, 'outside the epilogue-alone bound', ra)
    record(family + ' epilogue alone', tag, ra)
    # halo rows: the bits of the frame they mirror, or zero; masked frames: zero bits
    hb, lb = hi.bits(), (lo.bits() if lo is not None else None)
    src = ref['src']
    lims = R.lens_limits(c.N, c.Tout, S.D['fused'][f.name]['lens'])
    for rrow in range(rows):
        for b in (hb, lb):
            if b is None:
                continue
            if src[rrow] < 0:
                assert not b[:, rrow].any(), (tag, rrow, 'a zero halo row')
            else:
                assert np.array_equal(b[:, rrow], b[:, f.pad_l + src[rrow]]), (tag, rrow, 'a halo row differs from its frame')
    for n, lim in enumerate(lims):
        for b in (hb, lb):
            assert b is None or not b[n, f.pad_l + lim: f.pad_l + c.Tout].any(), (tag, n, 'a masked frame is not zero bits')
    for name, b in bad.items():
        assert ratio(got, b.v[:, :rows], redepth(b, 0, c.K).bound(r_out)[:, :rows]) > 1, (tag, name, 'the device agrees with a planted defect')
    return True


# ================================================================================================================================

@pytest.mark.parametrize('c', CONV_CASES, ids=lambda c: c.name)
def test_forward_against_float64(L, c):
    """every case under five shapes on slot rows and, where a shape has them, on tile rows; stride 2 is built for the 128x128
    shape alone, so case B also takes that shape's other K-loop structure and a split of it"""
    S = _setup(L, c)
    ran = 0
    for idx in FIVE + STRIDE2_MORE * (c.stride == 2):
        ran += check_plain(L, S, idx, SLOT_ROWS, 'conv fwd')
        if cols(idx) in (128, 256):
            ran += check_plain(L, S, idx, TILE_ROWS, 'conv fwd')
    assert ran == (6 if c.stride == 2 else 8), ran
    if c.stride == 2:
        assert plan(L, c, SLOT_ROWS, 2 + BASE, S.ws.numel())[0] == 2, 'the stride-2 split is real'


def test_every_configuration_on_slot_rows(L):
    """case E: all 52 unsplit indices, every fifth split-K / stream-K index; only launches that w2l_conv_plan says really split are
    counted as such (an infeasible split silently degrades to one block per tile)"""
    c = CONV_E
    S = _setup(L, c)
    ran = split = sk = 0
    for idx in list(range(BASE)) + list(range(BASE, 8 * BASE, 5)):
        if check_plain(L, S, idx, SLOT_ROWS, 'conv fwd sweep'):
            ran += 1
            blocks, ranges = plan(L, c, SLOT_ROWS, idx, S.ws.numel())
            split += idx >= BASE and blocks > 1
            sk += ranges > 0
    # (no stream-K on E: 18 tiles x 28 steps is below eight steps per range, so those indices pin the fall-back; case F below)
    assert ran >= 50 + R.E_SPLIT_FLOOR and split == R.E_SPLIT_FLOOR and sk == R.E_STREAMK_FLOOR == 0, (ran, split, sk)


def test_stream_k_that_really_runs(L):
    """case F (E's geometry, 13 utterances): every stream-K index whose plan has stream-K blocks (out[3] > 0), on slot rows and, for
    the 128- / 256-column shapes, on tile rows: a block then walks several tiles and runs the epilogue for each tile it finishes"""
    c = R.CONV_SK
    S = _setup(L, c)
    ran = 0
    for idx in range(STREAM_K, STREAM_K + BASE):
        for kind in (SLOT_ROWS, TILE_ROWS):
            if cannot_run(c, idx, kind):
                continue
            really = plan(L, c, kind, idx, S.ws.numel())
            if really[1] > 0:
                assert check_plain(L, S, idx, kind, 'conv fwd stream-K'), (idx, last_error(L))
                ran += 1
    assert ran == R.SK_FLOOR, ran


def test_tile_rows_on_every_128_and_256_column_shape(L):
    """case A (141 columns: the second half of a 256-column block's tile is partly dead): every 128- / 256-column shape writes one
    row per 128-column tile; a 144-column shape is an error and launches nothing"""
    S = _setup(L, CONV_A)
    ran = 0
    for idx in range(BASE):
        if cols(idx) in (128, 256):
            ran += check_plain(L, S, idx, TILE_ROWS, 'conv fwd tiles')
    assert ran == 26, ran
    assert cols(7) == 144 and not check_plain(L, S, 7, TILE_ROWS, 'conv fwd tiles')


def test_wholly_dead_second_half_of_a_256_column_tile(L):
    """case E on tile rows: 300 columns are 3 tiles of 128, so the last 256-column block's second half (trow 3) owns no row"""
    S = _setup(L, CONV_E)
    assert -(-CONV_E.Tout // 128) == 3 and -(-CONV_E.Tout // 256) * 2 == 4
    for idx in (12, 14 + NSHAPES, 2):
        assert check_plain(L, S, idx, TILE_ROWS, 'conv fwd tiles'), (idx, last_error(L))


@pytest.mark.parametrize('c', [CONV_A, CONV_E], ids=lambda c: c.name)
def test_three_pass_accumulate(L, c):
    """the fp32 mode's sequence hi*hi (+ bias), hi*lo, lo*hi with accumulate = 1 and the statistics on the third pass: the third
    launch against the reference whose acc_in is what the second left (an exact fp32 input), the end against all three products"""
    S = _setup(L, c)
    D = S.D
    if S.x_lo is None:
        S.x_lo, S.w_lo = up(D['x_lo'], torch.bfloat16), up(np.ascontiguousarray(D['w_lo'].transpose(2, 0, 1)), torch.bfloat16)
    xv = lambda a: a[:c.N * c.per].reshape(c.N, c.per, c.Cin)
    for idx, kind in ((2, SLOT_ROWS), (12 + NSHAPES, TILE_ROWS), (2 + 2 * BASE, SLOT_ROWS)):
        if cannot_run(c, idx, kind):
            continue
        rc, y = conv(L, S, idx, 1)
        assert rc == 0, last_error(L)
        rc, y = conv(L, S, idx, 1, y=y, accumulate=1, w=S.w_lo, bias=None)
        assert rc == 0, last_error(L)
        y2 = y.np().copy()
        pb, rows = S.partial(kind)
        rc, y = conv(L, S, idx, 1, kind, pb, y=y, accumulate=1, x=S.x_lo, bias=None)
        assert rc == 0, last_error(L)
        assert guards(y, pb, *S.inputs()) and not S.ws[:65536].any()
        yh = y.np()
        v3 = R.conv_fwd_ref(xv(D['x_lo']), D['w'], None, c.Tout, c.stride, c.dil, acc_in=y2)
        assert v3.d == c.K + 1
        r = record('conv fwd accumulate, third pass', f'{c.name} idx {idx}', ratio(yh, v3.v, redepth(v3, 0, c.K).bound()))
        assert r <= 1, (c.name, idx, r)
        p1 = R.conv_fwd_ref(xv(D['x']), D['w'], D['bias'], c.Tout, c.stride, c.dil)
        p2 = R.conv_fwd_ref(xv(D['x']), D['w_lo'], None, c.Tout, c.stride, c.dil)
        p3 = R.conv_fwd_ref(xv(D['x_lo']), D['w'], None, c.Tout, c.stride, c.dil)
        end = Tr(p1.v + p2.v + p3.v, p1.a + p2.a + p3.a, c.K + 3)           # bias, then one addition per accumulate launch
        r = record('conv fwd accumulate, three passes', f'{c.name} idx {idx}', ratio(yh, end.v, redepth(end, 0, c.K).bound()))
        assert r <= 1, (c.name, idx, r)
        got = sums_of(S, pb, rows, idx, kind)
        full = dict(zip(('s1', 's2'), R.conv_stats_ref(v3)))
        check_sums(S, got, idx, kind, yh, full, 'conv fwd accumulate', 'third pass')
        depth = R.stats_sum_depth(idx, c.N, c.Tout, SLOTS if kind == SLOT_ROWS else 0)
        bad = R.conv_stats_ref(v3, defect='acc_in_not_in_stats', acc_in=y2)
        assert not all(ratio(got[k], redepth(bad[k], depth, dot).v, redepth(bad[k], depth, dot).bound()) <= 1
                       for k, dot in enumerate((c.K, 2 * c.K))), (c.name, idx, 'the sums leave the accumulate operand out')


def test_two_launches_add_onto_the_same_slot_rows(L):
    c = CONV_D
    S = _setup(L, c)
    pb, rows = S.partial(SLOT_ROWS)
    for idx in (2, 21):
        rc, y = conv(L, S, idx, 1, SLOT_ROWS, pb)
        assert rc == 0, last_error(L)
    assert guards(y, pb, *S.inputs())
    got = sums_of(S, pb, rows, 2, SLOT_ROWS, launches=2)
    deeper = 21 if R.stats_sum_depth(21, c.N, c.Tout, SLOTS, 2) > R.stats_sum_depth(2, c.N, c.Tout, SLOTS, 2) else 2
    check_sums(S, got, deeper, SLOT_ROWS, None, S.ref, 'conv fwd two launches', 'added', launches=2, scale=2)
    one = [redepth(S.ref[s], R.stats_sum_depth(deeper, c.N, c.Tout, SLOTS, 2), dot) for s, dot in (('s1', c.K), ('s2', 2 * c.K))]
    assert ratio(got[0], one[0].v, one[0].bound()) > 1 and ratio(got[1], one[1].v, one[1].bound()) > 1, 'one launch alone'


def test_tuner_then_unforced_launch(L):
    """the measuring launches add onto scratch rows; the launch that follows takes the index w2l_conv_plan names.
    The measured choice stays in the library's process-wide table under case C's shape and statistics flag 2 for the rest of the
    session: no other test may rely on the cost model's choice for that key (every other launch of this file forces its index)."""
    c = CONV_C
    S = _setup(L, c)
    scratch, _ = S.partial(SLOT_ROWS)
    rc, ytune = conv(L, S, -1, 0, SLOT_ROWS, scratch, tune_reps=2)
    assert rc == 0, last_error(L)
    out = (ctypes.c_int * 8)()
    assert L.lib.w2l_conv_plan(c.N, c.Cin, c.Cout, c.Tout, c.Kw, c.stride, c.dil, SLOT_ROWS, S.ws.numel(), -1, out) == 0 and out[7] == 1
    idx = out[0]
    pb, rows = S.partial(SLOT_ROWS)
    rc, y32 = conv(L, S, -1, 1, SLOT_ROWS, pb)
    assert rc == 0, last_error(L)
    rc, y16 = conv(L, S, -1, 0, SLOT_ROWS, S.partial(SLOT_ROWS)[0])
    assert rc == 0, last_error(L)
    assert not S.ws[:65536].any() and guards(y32, y16, ytune, pb, scratch, *S.inputs())
    yh = y32.np()
    rc, forced = conv(L, S, idx, 1)
    assert rc == 0 and np.array_equal(forced.np().view(np.uint32), yh.view(np.uint32)), (idx, 'not the configuration the plan names')
    r = record('conv fwd tuned fp32 store', f'{c.name} idx {idx}', ratio(yh, S.ref['v'].v, redepth(S.ref['v'], 0, c.K).bound()))
    assert r <= 1, (idx, r)
    assert same_bits(y16, bf16_rne(yh))
    check_sums(S, sums_of(S, pb, rows, idx, SLOT_ROWS), idx, SLOT_ROWS, yh, S.ref, 'conv fwd tuned', 'slots')


VARIANTS = [(c, f) for c in CONV_CASES for f in c.fused]


@pytest.mark.parametrize('c,f', VARIANTS, ids=lambda v: v.name)
def test_fused_inference_against_float64(L, c, f):
    """every variant under the five shapes and one split index; the split must be real wherever the K loop is long enough"""
    S = _setup(L, c)
    ran = 0
    for idx in FIVE + (2 + BASE,) + STRIDE2_MORE[:1] * (c.stride == 2):
        ran += check_fused(L, S, f, idx, 'fused inference')
    assert ran == (3 if c.stride == 2 else 6), ran
    really = plan(L, c, FUSED, 2 + BASE, S.ws.numel())
    assert (really[0] == 2) == ((c.Cin // 64) * c.Kw >= 4), (c.name, really, 'two blocks per tile need four K steps')


def test_fused_inference_on_every_unsplit_configuration(L):
    c, f = CONV_A, CONV_A.fused[0]
    S = _setup(L, c)
    ran = sum(check_fused(L, S, f, idx, 'fused inference sweep') for idx in range(BASE))
    assert ran == 50, ran                # all but the spilling shape under both K-loop structures


def test_fused_inference_without_a_workspace(L):
    """w2l_conv1d_igemm_bnact (no workspace): a split index degrades to one block per tile"""
    c, f = CONV_D, CONV_D.fused[0]
    S = _setup(L, c)
    rc, hi, _ = fused(L, S, f, 2 + BASE, use_ws=False)
    assert rc == 0, last_error(L)
    rc, hi1, _ = fused(L, S, f, 2)
    assert rc == 0 and np.array_equal(hi.bits(), hi1.bits())


def test_argument_checks(L):
    """host side: every one of these returns an error and launches nothing"""
    c = CONV_A
    S = _setup(L, c)
    f = c.fused[0]
    S.fused_ops(f)
    plain = [
        ('Cin no multiple of 64', 'Cin=32 must be', dict(Cin=c.Cin - 32)),
        ('Cout no multiple of 64', 'Cout=160 must be', dict(Cout=c.Cout - 32)),
        ('stride 3', 'stride must be 1 or 2', dict(stride=3)),
        ('accumulate with a bf16 store', 'accumulate needs fp32', dict(y_f32=0, accumulate=1)),
        ('x_bstride no multiple of Cin', 'x_bstride must be', dict(x_bstride=c.per * c.Cin + 8)),
        ('a padded input one row too small', 'padded input too small', dict(x_rows_total=(c.N - 1) * c.per + c.need - 1)),
    ]
    for what, says, over in plain:
        pb, rows = S.partial(SLOT_ROWS)
        acc, y_f32 = over.pop('accumulate', 0), over.pop('y_f32', 1)
        y = Buf((c.N, c.Tout, c.Cout), torch.float32 if y_f32 else torch.bfloat16)
        rc, _ = conv(L, S, 2, y_f32, SLOT_ROWS, pb, y=y, accumulate=acc, **over)
        assert rc != 0 and says in last_error(L), (what, last_error(L))
        assert torch.isnan(y.t).all() and unwritten(pb, rows, SLOT_ROWS) and guards(y, pb), (what, 'something was launched')
    assert conv(L, S, 2, 1, SLOT_ROWS, S.partial(SLOT_ROWS)[0], x_rows_total=(c.N - 1) * c.per + c.need)[0] == 0, 'exactly enough rows run'
    rows = f.pad_l + c.Tout + f.pad_r
    dummy = Buf((c.N, c.Tout, c.Cout), torch.bfloat16)
    # case D (19 frames) for the reflect condition: on case A a pad of Tout = 141 is above 96 and never reaches it
    cd, fd = CONV_D, CONV_D.fused[0]
    Sd = _setup(L, cd)
    Sd.fused_ops(fd)
    fz = [
        (S, f, 'a pad above 96', 'bad output geometry', dict(epi=dict(pad_mode=0, pad_l=97, out_rows=rows + 200))),
        (Sd, fd, 'a reflect pad_r of Tout', 'reflect pad', dict(epi=dict(pad_mode=1, pad_l=3, pad_r=cd.Tout))),
        (Sd, fd, 'a reflect pad_l of Tout', 'reflect pad', dict(epi=dict(pad_mode=1, pad_l=cd.Tout, pad_r=3))),
        (S, f, 'out_rows one short', 'bad output geometry', dict(epi=dict(out_rows=rows - 1))),
        (S, f, 'res_lo without res', 'res_lo needs res', dict(epi=dict(res=None, res_lo=addr(dummy)))),
        (S, f, 'Cout no multiple of 64', 'multiple of 64', dict(Cout=c.Cout - 32)),
        (S, f, 'a padded input one row too small', 'padded input too small', dict(x_rows_total=(c.N - 1) * c.per + c.need - 1)),
    ]
    for Sx, fx, what, says, over in fz:
        rc, hi, _ = fused(L, Sx, fx, 2, **over)
        assert rc != 0 and says in last_error(L), (what, last_error(L))
        assert torch.isnan(hi.t).all() and guards(hi), (what, 'something was launched')
    # the nearest values that are allowed run
    assert fused(L, S, f, 2)[0] == 0, 'the same call without a fault runs'
    assert fused(L, S, f, 2, epi=dict(pad_mode=0, pad_l=96, out_rows=96 + c.Tout + f.pad_r))[0] == 0, (last_error(L), 'a pad of 96 runs')
    for pads in (dict(pad_l=3, pad_r=cd.Tout - 1), dict(pad_l=cd.Tout - 1, pad_r=3)):
        rc, hi, _ = fused(L, Sd, fd, 2, epi=dict(pad_mode=1, **pads))
        assert rc == 0 and guards(hi), (pads, last_error(L), 'a reflect pad of Tout - 1 runs')
