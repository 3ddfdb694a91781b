"""w2l_conv1d_dgrad_bnreduce_ws (conv_igemm_kernel<.., EPI = 1>: the flat data gradient with the BatchNorm-backward reduce of the
producer layer in its epilogue) called directly, against bn_refs.dgrad_bnreduce_ref (float64; pinned by
tests/test_cpu_dgrad_bnreduce_refs.py, which also proves that the planted defects exceed the bound of every case below that they
can show on).  Per launch:

  1. dxp is bit-identical to w2l_conv1d_igemm_ws (bf16 store, no statistics) on the same operands under the same forced
     configuration: the epilogue does not change the store;
  2. the column sums of the partial rows lie within Tr.bound of the reference's sums, per channel (dot product of depth Kw Cout,
     one product with gk, xhat and its product, a row sum as deep as there are padded rows); rows the launch does not own stay as
     they were;
  3. unsplit configurations: with the fp32 accumulators of the plain y_f32 = 1 launch of the same configuration taken as EXACT
     inputs, the sums lie within the bound of the epilogue alone -- no dot-product term, so nothing about the matrix unit enters;
  4. the device's sums violate the bound of every planted-defect reference (bn_refs.DG_DEFECTS) that applies to the case.

DOT_MARGIN is the one number not derived: the factor on the dot-product term of bound 2, 1 while the plain data gradient obeys
(Kw Cout + 2) u A (test_plain_data_gradient_obeys_its_bound measures and asserts exactly that).
This file sets the statistics mode and forces configurations; both are thread-local hooks and are reset after every launch."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import bn_refs as B
from bn_refs import Tr, U
from direct_helpers import Buf, guards, last_error, ratio, record

pytestmark = pytest.mark.gpu

SLOTS = 8
DOT_MARGIN = 1.0
# the block shapes (mw, nw, ms, ns) of conv_igemm.hip in index order: BM = 16 mw ms channels x BN = 16 nw ns rows
SHAPES = [(2, 2, 2, 4), (2, 2, 3, 4), (2, 2, 4, 4), (2, 2, 5, 4), (4, 2, 3, 4), (4, 2, 4, 4), (2, 3, 2, 3), (2, 3, 3, 3), (2, 3, 4, 3),
          (2, 3, 5, 3), (2, 4, 2, 4), (2, 4, 3, 4), (2, 4, 4, 4), (2, 4, 5, 4), (2, 4, 6, 4), (2, 4, 7, 4), (2, 4, 8, 4), (2, 3, 4, 6),
          (2, 3, 5, 6), (2, 3, 6, 6), (2, 3, 7, 6), (2, 4, 4, 6), (2, 4, 5, 6), (2, 4, 6, 6), (2, 4, 4, 7), (2, 4, 5, 7)]
NSHAPES, SPILL, LDS_BYTES = 26, 20, 160 * 1024
BASE = 2 * NSHAPES                      # an index is shape + 26 * K-loop structure + 52 * split option
STREAM_K = 7 * BASE


def cols(idx):
    _, nw, _, ns = SHAPES[idx % NSHAPES]
    return 16 * nw * ns


def lds_fits(idx, hb):
    mw, nw, ms, ns = SHAPES[idx % NSHAPES]
    xrows = (16 * nw * ns - 1 + hb + 1 + 7) & ~7
    return 2 * 16 * mw * ms * 128 + 2 * xrows * 128 <= LDS_BYTES


@pytest.fixture(scope='module')
def L():
    from wav2letter_pytorch_amd import _lib
    assert torch.cuda.is_available()
    return _lib


def addr(b):
    return None if b is None else b.t.data_ptr()


def up(a, dtype=torch.float32):
    return None if a is None else Buf(a.shape, dtype, torch.from_numpy(np.ascontiguousarray(a)))


def wait(what):
    """a HIP error ends the session: nothing more is launched on a device that has faulted"""
    try:
        torch.cuda.synchronize()
    except Exception as e:                              # noqa: BLE001
        pytest.exit(f'HIP error in {what}, nothing more is run: {e}', returncode=3)


class Setup:
    """device copies of a case (and of the other consumer's dy and w: variant 1), its references, its workspace"""

    def __init__(self, L, g):
        self.g, c = g, g.u
        self.D = D = B.make_dg_case(g)
        self.ops = {0: self._operands(D)}
        self.y = up(D['y'], torch.bfloat16)
        self.scale, self.shift, self.mean, self.invstd = (up(D[k]) for k in ('scale', 'shift', 'mean', 'invstd'))
        self.lens = up(D['lens'], torch.int32)
        m = D['mask']
        if m is not None and D['lens'] is not None:     # what the forward pass leaves: the bytes of frames t >= lens[n] unwritten
            m = m.copy().reshape(c.N, c.T, c.G)
            for n, lim in enumerate(B.lens_limits(c.N, c.T, D['lens'])):
                m[n, lim:] = 0xA5
        self.mask = up(m, torch.uint8)
        self.ws = torch.zeros(int(L.lib.w2l_conv_splitk_workspace_bytes(1, c.C, g.flat_rows)), dtype=torch.uint8, device='cuda')
        self.ref = B.dg_ref_of(g, D)
        self.bad = {d: B.dg_ref_of(g, D, defect=d)['sums'] for d in B.DG_DEFECTS if B.dg_defect_applies(g, d)}

    def _operands(self, D):
        w_dgr = np.ascontiguousarray(D['w'][:, :, ::-1].transpose(2, 1, 0))          # [Kw][C][Cout], taps flipped
        return up(D['dy'], torch.bfloat16), up(w_dgr, torch.bfloat16)

    def variant(self, v):
        if v not in self.ops:
            self.ops[v] = self._operands(B.make_dg_case(self.g, v))
        return self.ops[v]

    def inputs(self):
        return [b for pair in self.ops.values() for b in pair] + [self.y, self.scale, self.shift, self.mean, self.invstd, self.lens,
                                                                  self.mask]

    def desc(self, L, **over):
        c, D = self.g.u, self.D
        d = L.BnActDesc(N=c.N, T=c.T, C=c.C, y=addr(self.y), y_f32=0, scale=addr(self.scale), shift=addr(self.shift),
                        mean=addr(self.mean), invstd=addr(self.invstd), y2=None, scale2=None, shift2=None, mean2=None, invstd2=None,
                        act=c.act, drop_p=c.p, seed=D['seed'], offset=D['offset'], mask=addr(self.mask), lens=addr(self.lens),
                        offset_dev=None, q_clipped=None)
        for k, v in over.items():
            setattr(d, k, v)
        return d

    def dy_args(self, v=0):
        """(pointer at row halo - hb, rows readable from there) of the shared-halo buffer"""
        g = self.g
        dy, _ = self.variant(v)
        return ctypes.c_void_p(dy.t.data_ptr() + (g.halo - g.hb) * g.Cout * 2), g.hb + g.flat_rows

    def partial(self, mode):
        """mode S: S zero rows (the kernel adds) then 2 NaN rows; mode 0: one NaN row per 128-row tile then 2 more"""
        g = self.g
        rows = mode if mode else -(-g.flat_rows // 128)
        pb = Buf((rows + 2, 2, g.u.C))
        if mode:
            pb.t[:rows].zero_()
        return pb, rows


@functools.lru_cache(maxsize=None)
def _setup(L, g):
    return Setup(L, g)


def fused(L, S, idx, mode, pb, v=0, tune_reps=0, **over):
    """one launch (or the tuner) under the statistics mode and the forced configuration; returns (rc, dxp)"""
    g = S.g
    dxp = Buf((g.flat_rows, g.u.C), torch.bfloat16)
    d = S.desc(L, **over.pop('desc', {}))
    ptr, rows_total = S.dy_args(v)
    a = dict(pad_l=g.u.pad_l, pad_r=g.u.pad_r, pad_mode=g.u.pad_mode, per=g.per, flat_rows=g.flat_rows,
             partial=None if pb is None else L.ptr(pb.t), d=ctypes.byref(d))
    a.update(over)
    head = (ptr, rows_total, L.ptr(S.variant(v)[1].t), L.ptr(dxp.t), a['partial'], a['d'], a['pad_l'], a['pad_r'], a['pad_mode'],
            a['per'], g.Cout, a['flat_rows'], g.Kw, g.dil)
    tail = (L.ptr(S.ws), S.ws.numel(), L.stream_ptr())
    L.lib.w2l_conv_force_tile_config(idx)
    L.lib.w2l_conv_stats_mode(mode)
    try:
        if tune_reps:
            rc = L.lib.w2l_conv1d_dgrad_bnreduce_tune_ws(*head, tune_reps, *tail)
        else:
            rc = L.lib.w2l_conv1d_dgrad_bnreduce_ws(*head, *tail)
    finally:
        L.lib.w2l_conv_stats_mode(0)
        L.lib.w2l_conv_force_tile_config(-1)
    wait('a fused data-gradient launch')
    return rc, dxp


def plain(L, S, idx, y_f32, v=0):
    """w2l_conv1d_igemm_ws(N = 1, Tout = flat_rows) on the same operands: no statistics, bf16 or fp32 store"""
    g = S.g
    y = Buf((g.flat_rows, g.u.C), torch.float32 if y_f32 else torch.bfloat16)
    ptr, rows_total = S.dy_args(v)
    L.lib.w2l_conv_force_tile_config(idx)
    try:
        rc = L.lib.w2l_conv1d_igemm_ws(ptr, rows_total * g.Cout, rows_total, L.ptr(S.variant(v)[1].t), L.ptr(y.t), y_f32, 0, None, None,
                                       1, g.Cout, g.u.C, g.flat_rows, g.Kw, 1, g.dil, L.ptr(S.ws), S.ws.numel(), L.stream_ptr())
    finally:
        L.lib.w2l_conv_force_tile_config(-1)
    wait('a plain data-gradient launch')
    assert rc == 0, (idx, last_error(L))
    return y


def sums_bound(g, tr):
    """Tr.bound with DOT_MARGIN on the dot product's share of the depth"""
    dot = g.Kw * g.Cout
    assert tr.d - dot + DOT_MARGIN * dot < 5000
    return (DOT_MARGIN * dot + tr.d - dot + 2) * U * tr.a


def same_bits(a, b):
    return torch.equal(a.t.view(torch.int16), b.t.view(torch.int16))


def owned_rows(g, idx, mode, rows):
    """partial rows a launch writes: row (column tile mod S) under mode S, every 128-row tile's under mode 0"""
    return min(rows, -(-g.flat_rows // cols(idx))) if mode else rows


def check_launch(L, S, idx, mode, family):
    """assertions 1-4 on one forced configuration; False: the configuration cannot run this problem (for a documented reason)"""
    g = S.g
    pb, rows = S.partial(mode)
    rc, dxp = fused(L, S, idx, mode, pb)
    if rc != 0:
        why = last_error(L)
        assert idx % NSHAPES == SPILL or not lds_fits(idx, g.hb) or (mode == 0 and cols(idx) not in (128, 256)), (idx, why)
        untouched = torch.isnan(pb.t[rows:]).all() and (not pb.t[:rows].any() if mode else torch.isnan(pb.t[:rows]).all())
        assert torch.isnan(dxp.t).all() and untouched, (idx, 'an error was returned and something was launched')
        return False
    assert guards(dxp, pb, *S.inputs()), idx
    assert not S.ws[:65536].any(), (idx, 'split-K tickets must be back at zero')
    # 1. the store (a stream-K index falls back to one block per tile under an epilogue: compared with that launch)
    pidx = idx - STREAM_K if idx >= STREAM_K else idx
    assert same_bits(dxp, plain(L, S, pidx, 0)), (idx, 'dxp differs from the plain launch')
    # 2. the sums, independently
    part = pb.np().astype(np.float64)
    own = owned_rows(g, idx, mode, rows)
    assert np.isfinite(part[:own]).all() and np.isnan(part[rows:]).all(), idx
    assert mode == 0 or not part[own:rows].any(), (idx, 'a slot row beyond the column tiles was written')
    got = part[:rows].sum(0)
    want = S.ref['sums']
    r2 = ratio(got, want.v, sums_bound(g, want))
    print(f'{g.name} idx {idx} mode {mode}: sums error / bound {r2:.2e}')
    assert r2 <= 1, (g.name, idx, mode, r2)
    record(family + ' sums', f'{g.name} idx {idx} mode {mode}', r2)
    if not g.u.bn1:
        assert not got[1].any(), 'a unit without BatchNorm: the second sum is exactly 0'
    # 3. the epilogue alone, on the accumulators of the plain fp32 launch of the same configuration
    if idx < BASE:
        acc = plain(L, S, idx, 1).np().astype(np.float64)
        alone = B.dg_ref_of(g, S.D, dx=acc)
        r3 = ratio(got, alone.v, alone.bound())
        assert r3 <= 1, (g.name, idx, mode, r3)
        record(family + ' epilogue alone', f'{g.name} idx {idx} mode {mode}', r3)
    # 4. sensitivity
    for name, bad in S.bad.items():
        assert ratio(got, bad.v, sums_bound(g, bad)) > 1, (g.name, idx, name, 'the device agrees with a planted defect')
    return True


# ================================================================================================================================

@pytest.mark.parametrize('g', B.DG_CASES, ids=lambda g: g.name)
def test_plain_data_gradient_obeys_its_bound(L, g):
    """the premise of bound 2: the fp32 accumulators of the matrix unit obey (Kw Cout + 2) u A (times DOT_MARGIN)"""
    S = _setup(L, g)
    worst = 0.0
    for idx in (2, 12, 7 + NSHAPES, 24):
        acc = plain(L, S, idx, 1).np()
        dx = S.ref['dx']
        worst = max(worst, ratio(acc, dx.v, dx.bound()))
    record('dgrad plain fp32', g.name, worst)
    assert worst <= DOT_MARGIN, worst


@pytest.mark.parametrize('g', B.DG_CASES, ids=lambda g: g.name)
def test_fused_against_float64(L, g):
    """every case under slot rows (a 128-, an 8-wave 128-, a 256-, a 144- and a 448-column shape; both K-loop structures) and
    under one row per 128-row tile (a 128- and a 256-column shape)"""
    S = _setup(L, g)
    for idx in (2, 5 + NSHAPES, 12, 7, 24 + NSHAPES):
        assert check_launch(L, S, idx, SLOTS, 'dgrad+bnreduce'), (idx, last_error(L))
    for idx in (2 + NSHAPES, 12):
        assert check_launch(L, S, idx, 0, 'dgrad+bnreduce'), (idx, last_error(L))


def test_every_block_shape_on_slot_rows(L):
    """w2l_conv_stats_mode(8), case B: every block shape x both K-loop structures, every fifth split-K / stream-K index"""
    S = _setup(L, B.DG_B)
    ran = wide = 0
    for idx in list(range(BASE)) + list(range(BASE, BASE * 8, 5)):
        if check_launch(L, S, idx, SLOTS, 'dgrad+bnreduce sweep'):
            ran += 1
            wide += cols(idx) not in (128, 256)
    assert ran >= 90 and wide >= 40, (ran, wide)


def test_128_column_tiles_without_slot_rows(L):
    """mode 0, case A (per = 153: utterances straddle tiles and fragments): the shapes of 128 and 256 columns write one row per
    128-row tile; a 144-column shape is an error and launches nothing"""
    S = _setup(L, B.DG_A)
    ran = 0
    for idx in range(BASE):
        if cols(idx) in (128, 256):
            ran += check_launch(L, S, idx, 0, 'dgrad+bnreduce tiles')
    assert ran == 26, ran
    assert cols(7) == 144 and not check_launch(L, S, 7, 0, 'dgrad+bnreduce tiles')


def test_two_consumers_add_onto_the_same_rows(L):
    """a residual branch: two fused launches with different dy and w add onto the same slot rows"""
    g = B.DG_B
    S = _setup(L, g)
    pb, rows = S.partial(SLOTS)
    for v, idx in ((0, 2), (1, 21)):
        rc, dxp = fused(L, S, idx, SLOTS, pb, v=v)
        assert rc == 0, last_error(L)
        assert same_bits(dxp, plain(L, S, idx, 0, v=v))
    refs = [S.ref['sums'], B.dg_ref_of(g, B.make_dg_case(g, 1))['sums']]
    want = refs[0] + refs[1]
    got = pb.np().astype(np.float64)[:rows].sum(0)
    r = record('dgrad+bnreduce two consumers', g.name, ratio(got, want.v, sums_bound(g, want)))
    assert r <= 1, r
    assert ratio(got, refs[0].v, sums_bound(g, refs[0])) > 1 and guards(pb, *S.inputs())


def test_tuner_then_launch(L):
    """the measuring launches add onto scratch rows; the launch that follows takes the remembered configuration"""
    g = B.DG_C
    S = _setup(L, g)
    scratch, _ = S.partial(SLOTS)
    rc, _ = fused(L, S, -1, SLOTS, scratch, tune_reps=2)
    assert rc == 0, last_error(L)
    out = (ctypes.c_int * 8)()
    assert L.lib.w2l_conv_plan(1, g.Cout, g.u.C, g.flat_rows, g.Kw, 1, g.dil, 2, S.ws.numel(), -1, out) == 0 and out[7] == 1
    idx = out[0]
    pb, rows = S.partial(SLOTS)
    rc, dxp = fused(L, S, -1, SLOTS, pb)
    assert rc == 0, last_error(L)
    assert not S.ws[:65536].any() and guards(dxp, pb, scratch, *S.inputs())
    assert same_bits(dxp, plain(L, S, idx, 0)), (idx, 'not the remembered configuration, or the store differs')
    got = pb.np().astype(np.float64)[:rows].sum(0)
    r = record('dgrad+bnreduce tuned', f'{g.name} idx {idx}', ratio(got, S.ref['sums'].v, sums_bound(g, S.ref['sums'])))
    assert r <= 1, (idx, r)


def test_argument_checks(L):
    """host side: every one of these returns an error and launches nothing"""
    g = B.DG_B
    S = _setup(L, g)
    c = g.u
    f32y = Buf((c.N, c.T, c.C))
    bad = [
        ('an fp32 y', dict(desc=dict(y_f32=1, y=addr(f32y)))),
        ('a residual descriptor', dict(desc=dict(y2=addr(S.y)))),
        ('dropout without a mask', dict(desc=dict(mask=None))),
        ('per below the padded rows', dict(per=g.Tp - 1, flat_rows=c.N * (g.Tp - 1))),
        ('C no multiple of 64', dict(desc=dict(C=c.C - 32))),
        ('a NULL partial', dict(partial=None)),
        ('flat_rows above N per', dict(desc=dict(N=c.N - 1))),
        ('flat_rows below N per', dict(flat_rows=g.flat_rows - g.per)),
        ('a NULL descriptor', dict(d=None)),
    ]
    for what, over in bad:
        pb, rows = S.partial(SLOTS)
        rc, dxp = fused(L, S, 2, SLOTS, pb, **over)
        assert rc != 0, what
        assert 'conv1d_dgrad_bnreduce' in last_error(L) or 'multiple of 64' in last_error(L), (what, last_error(L))
        assert torch.isnan(dxp.t).all() and not pb.t[:rows].any() and guards(dxp, pb), (what, 'something was launched')
    pb, rows = S.partial(SLOTS)
    assert fused(L, S, 2, SLOTS, pb)[0] == 0, 'the same call without a fault runs'
