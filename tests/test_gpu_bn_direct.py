"""Every entry point of csrc/bn_act.hip called directly, each against its float64 reference (tests/bn_refs.py, itself pinned by
tests/test_cpu_bn_refs.py) under the derived per-element bound |got - ref| <= (d + 2) u A + r_out |ref| (kernel_refs.py), with
r_out = 0 (fp32), 2^-8 (bf16), 2^-17 (hi+lo pair), and 2^-4 |ref qs| + 2^-10 + bound qs for an e4m3 copy.  Dropout masks must
be byte-equal to the Philox reference (frames t >= lens[n] excepted: the forward pass writes them as zeros without drawing their
bits, those bytes stay as they were, and the backward tests hand the backward kernels garbage there to show they are never used),
gates and the q_clipped count equal (the case generator leaves no ambiguous element).
Every output element is compared; outputs start as NaN (0xA5 bytes) and are followed by a guard region.

Which case reaches which kernel (thresholds: bn_act.hip):

  kernel family              entry point(s)                          cases                          why / threshold
  bn_finalize_kernel         w2l_bn_finalize                         test_bn_finalize               ntiles 1..121: 8 tile lanes, 64-step loop (l.1179)
  bn_act_fwd_kernel          w2l_bn_act_fwd, _fwd_q                  GENERAL (small), FWD_ONLY      grid = ceil(R*G / 256) x N (l.1318); G = 1, 3: the fix-up (l.192-194)
  bn_act_fwd_fin_kernel      w2l_bn_act_fwd_fin                      FWD_FIN_SMALL, FWD_FIN_BIG     fwd_rows_per_block (l.260-267): two batches from N*R*(C/64) > 81920
  quantize_e4m3_kernel       w2l_quantize_e4m3                       test_quantize                  elementwise_blocks (l.1223): 4096 blocks, then the grid stride
  quantize_e4m3_dyn_kernel   w2l_quantize_e4m3_dyn                   test_quantize_dyn              the same; amax binades exact (l.1157)
  bn_act_bwd_reduce_kernel   w2l_bn_act_bwd_reduce                   GENERAL                        bwd_rows_per_wave (l.712-719): 16 (clamp..), 24 (mid_rows), 64 (wide_rows)
  bn_bwd_finalize_kernel     w2l_bn_bwd_finalize                     GENERAL, test_bwd_finalize_rows 64-step loop, b + 56 < nblocks (l.787): 1, 9, 57, 64, 65
  bn_act_bwd_apply_kernel    w2l_bn_act_bwd_apply, _apply_amax       GENERAL (small), BIG_APPLY     elementwise_blocks: > 4096 x 256 items = a second round (l.820)
  bn_act_bwd_apply_fin_kernel w2l_bn_act_bwd_apply_fin               GENERAL, test_apply_fin_rows   apply_rows_per_block (l.885-889): 64, 160 (wide_rows); 16-step loop (l.910)
  bn_bwd_reduce_fast_kernel  w2l_bn_act_bwd_reduce_slots             SLOTS, LOOPED[2:]              bn_loop_iters == 0 (l.1412-1418); U = 2 (l.1432)
  bn_bwd_apply_fast_kernel   w2l_bn_act_bwd_apply_slots              SLOTS, LOOPED[2:]              U = 4 with amax, 2 for C <= 384 (u2, t5), else 1 (u1) (l.1459)
  bn_bwd_reduce_loop_kernel  w2l_bn_act_bwd_reduce_slots             LOOPED[:2]                     rows >= 12000 and rows * C >= 8 000 000 and T >= 8 (l.1414-1415)
  bn_bwd_apply_loop_kernel   w2l_bn_act_bwd_apply_slots              LOOPED[:2]                     the same
  (host)                     w2l_bn_bwd_blocks, w2l_bn_bwd_fast_ok   every case                     equal to the restated formulas

This file sets no chain setting, no statistics mode and no forced plan."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import bn_refs as B
from bn_refs import Tr
from direct_helpers import Buf, guards, last_error, p, ratio, record

pytestmark = pytest.mark.gpu

EPS, MOM = 1e-3, 0.1


@pytest.fixture(scope='module')
def L():
    from wav2letter_pytorch_amd import _lib
    assert torch.cuda.is_available()
    return _lib


def addr(b):
    return None if b is None else b.t.data_ptr()


def up(a, dtype=torch.float32):
    """a host array (or None) as a guarded device buffer"""
    return None if a is None else Buf(a.shape, dtype, torch.from_numpy(np.ascontiguousarray(a)))


class Dev:
    """the device copies of a case's inputs; every size comes from Case.sizes()"""

    def __init__(self, c, D):
        self.c, self.D = c, D
        s = c.sizes()
        ydt = torch.bfloat16 if not c.y_f32 else torch.float32
        gdt = torch.bfloat16 if not c.g_f32 else torch.float32
        self.y, self.y2 = up(D['y'], ydt), up(D['y2'], ydt)
        assert self.y.n == s['y']
        for k in ('scale', 'shift', 'mean', 'invstd', 'scale2', 'shift2', 'mean2', 'invstd2'):
            setattr(self, k, up(D[k]))
        self.lens = up(D['lens'], torch.int32)
        m = D['mask']
        if m is not None and D['lens'] is not None:     # what the forward pass leaves: the bytes of frames t >= lens[n] unwritten
            m = m.copy().reshape(c.N, c.T, c.G)
            for n, lim in enumerate(B.lens_limits(c.N, c.T, D['lens'])):
                m[n, lim:] = 0xA5
        self.mask = up(m, torch.uint8)
        assert self.mask is None or self.mask.n == s['mask']
        self.g = [up(g, gdt) for g, *_ in D['srcs']]
        assert self.g[0].n == s['src1'] and (len(self.g) == 1 or self.g[1].n == s['src2'])

    def inputs(self):
        return [self.y, self.y2, self.scale, self.shift, self.mean, self.invstd, self.scale2, self.shift2, self.mean2, self.invstd2,
                self.lens, self.mask] + self.g

    def desc(self, L, mask=None, **over):
        c, D = self.c, self.D
        d = L.BnActDesc(N=c.N, T=c.T, C=c.C, y=addr(self.y), y_f32=c.y_f32, scale=addr(self.scale), shift=addr(self.shift),
                        mean=addr(self.mean), invstd=addr(self.invstd), y2=addr(self.y2), scale2=addr(self.scale2),
                        shift2=addr(self.shift2), mean2=addr(self.mean2), invstd2=addr(self.invstd2), act=c.act, drop_p=c.p,
                        seed=D['seed'], offset=D['offset'], mask=addr(mask if mask is not None else self.mask), lens=addr(self.lens),
                        offset_dev=None, q_clipped=None)
        for k, v in over.items():
            setattr(d, k, v)
        return d

    def srcs(self, L):
        out = []
        for b, (g, pl, pr, pm) in zip(self.g, self.D['srcs']):
            out.append(L.GradSrc(dxp=addr(b), f32=self.c.g_f32, pad_l=pl, pad_r=pr, pad_mode=pm, rows=g.shape[1]))
        return out + [None] * (2 - len(out))


def run(L, rc):
    """check the launch and wait for it; a HIP error ends the session: nothing more is launched on a device that has faulted"""
    try:
        L.check(rc)
        torch.cuda.synchronize()
    except Exception as e:                              # noqa: BLE001
        pytest.exit(f'HIP error in a direct BatchNorm launch, nothing more is run: {e}', returncode=3)


def layout(x, N, T, h):
    """[N*T][C] frames -> the shared-halo layout [h + N*(T+h)][C], halo rows zero"""
    Cc = x.shape[-1]
    out = np.zeros((h + N * (T + h), Cc))
    x = x.reshape(N, T, Cc)
    for n in range(N):
        out[h + n * (T + h): h + n * (T + h) + T] = x[n]
    return out


def dy_ratio(hi, lo, tr, N, T, h):
    """a dy buffer (bf16 hi [+ lo]) against the reference frames ``tr`` (Tr of [N*T][C], halo = 0 layout)"""
    ref, a = layout(tr.v, N, T, h), layout(tr.a, N, T, h)
    t = Tr(ref, a, tr.d)
    r = ratio(hi.np(), ref, t.bound(B.R_BF16))
    if lo is not None:
        r = max(r, ratio(hi.np().astype(np.float64) + lo.np(), ref, t.bound(B.R_SPLIT)))
    return r


def amax_check(amax, rows_ref, what):
    """|max over slots - max |ref|| <= max bound, per row; rows_ref: [(Tr or None)] for row 0, row 1"""
    got = amax.np().reshape(2, B.AMAX_SLOTS)
    for k, tr in enumerate(rows_ref):
        if tr is None:
            assert not got[k].any(), f'{what}: amax row {k} must stay zero'
        else:
            assert abs(float(got[k].max()) - float(np.abs(tr.v).max())) <= float(tr.bound().max()), f'{what}: amax row {k}'


# ================================================================================================================================
# w2l_bn_finalize
# ================================================================================================================================

@pytest.mark.parametrize('Cc', [8, 40, 64, 100])
def test_bn_finalize(L, Cc):
    worst = 0.0
    rng = np.random.default_rng(Cc)
    for i, ntiles in enumerate([1, 7, 8, 57, 64, 121]):
        per = 1 if (ntiles == 1 and Cc == 8) else 5                      # count = 1: unbiased == biased
        pr, count = B.make_partial(ntiles, Cc, per, 10 * Cc + ntiles, const_channel=3 if per > 1 else None)
        ga = (rng.random(Cc) + 0.5).astype(np.float32) if i % 2 == 0 else None
        be = rng.standard_normal(Cc).astype(np.float32) if i % 3 != 1 else None
        rm = rng.standard_normal(Cc).astype(np.float32) if i % 4 != 3 else None
        rv = (rng.random(Cc) + 0.5).astype(np.float32) if rm is not None else None
        stats = i % 5 != 4                                                 # mean / invstd may be NULL
        ref = B.bn_finalize_ref(pr, Cc, count, ga, be, EPS, MOM, rm, rv)
        P_, Ga, Be, Rm, Rv = up(pr), up(ga), up(be), up(rm), up(rv)
        out = {k: Buf((Cc,)) for k in (('mean', 'invstd') if stats else ()) + ('scale', 'shift')}
        run(L, L.lib.w2l_bn_finalize(p(L, P_), ntiles, Cc, count, p(L, Ga), p(L, Be), EPS, MOM, p(L, Rm), p(L, Rv), p(L, out.get('mean')),
                                     p(L, out.get('invstd')), p(L, out['scale']), p(L, out['shift']), L.stream_ptr()))
        got = {k: b.np() for k, b in out.items()}
        if rm is not None:
            got.update(running_mean=Rm.np(), running_var=Rv.np())
        for k, v in got.items():
            r = ratio(v, ref[k].v, ref[k].bound())
            worst = max(worst, r)
            assert r <= 1, f'bn_finalize C={Cc} ntiles={ntiles} {k}: error / bound = {r}'
        if per > 1:
            assert ref['invstd'].v[3] == 1 / np.sqrt(B.f32(EPS)), 'the constant channel: var clamps at 0'
        assert guards(P_, Ga, Be, Rm, Rv, *out.values())
        # eval form: statistics from the running values
        if rm is not None:
            rm2, rv2 = Rm.np().copy(), Rv.np().copy()
            ev = B.bn_finalize_ref(None, Cc, 0, ga, be, EPS, MOM, rm2, rv2)
            eo = {k: Buf((Cc,)) for k in ('mean', 'invstd', 'scale', 'shift')}
            run(L, L.lib.w2l_bn_finalize(None, 0, Cc, 0, p(L, Ga), p(L, Be), EPS, MOM, p(L, Rm), p(L, Rv), p(L, eo['mean']), p(L, eo['invstd']),
                                         p(L, eo['scale']), p(L, eo['shift']), L.stream_ptr()))
            for k, b in eo.items():
                r = ratio(b.np(), ev[k].v, ev[k].bound())
                worst = max(worst, r)
                assert r <= 1, f'bn_finalize eval C={Cc} {k}: error / bound = {r}'
            assert np.array_equal(Rm.np(), rm2) and np.array_equal(Rv.np(), rv2) and guards(Rm, Rv, *eo.values())
    record('bn_finalize', f'C={Cc}', worst)


# ================================================================================================================================
# forward: w2l_bn_act_fwd / _fwd_q
# ================================================================================================================================

FWD_CASES = [c for c in B.GENERAL if not B.is_big(c)] + B.FWD_ONLY + B.SLOTS


def check_forward(c, fw, hi, lo, q, mask, clipped_before, qc, what):
    """outputs of a forward launch against the forward reference ``fw``; returns the worst ratio"""
    a = fw['a']
    r = ratio(hi.np(), a.v, a.bound(B.R_BF16))
    if lo is not None:
        r = max(r, ratio(hi.np().astype(np.float64) + lo.np(), a.v, a.bound(B.R_SPLIT)))
    assert r <= 1, f'{what}: activation error / bound = {r}'
    if c.p > 0:
        got, w = mask.np().reshape(-1), fw['mask_written']
        assert np.array_equal(got[w], fw['mask'][w]), f'{what}: mask bytes differ from keep_bits'
        assert (got[~w] == 0xA5).all(), f'{what}: the mask bytes of frames t >= lens[n] are not written'
    if q is not None:
        aq = fw['aq']
        rq = ratio(B.E4M3[q.np()], np.clip(aq.v, -448, 448), B.e4m3_bound(aq, c.q_scale))
        assert rq <= 1, f'{what}: e4m3 error / bound = {rq}'
        r = max(r, rq)
        if c.p in (0.0, 0.5):                           # z' of the planted channels is computed exactly: the codes are equal
            assert np.array_equal(q.np()[:, :, :4], fw['codes'][:, :, :4]), f'{what}: e4m3 codes of exact values'
        unsure = int((np.abs(fw['clip_margin']) <= fw['clip_bound']).sum())
        got = int(qc.np()[0]) - clipped_before
        assert fw['clipped'] - unsure <= got <= fw['clipped'] + unsure, f'{what}: q_clipped {got}, reference {fw["clipped"]} +- {unsure}'
    return r


@functools.lru_cache(maxsize=None)
def fwd_reference(c):
    return B.fwd_ref_of(c, B.make_case(c))


@pytest.mark.parametrize('c', FWD_CASES, ids=lambda c: c.name)
def test_bn_act_fwd(L, c):
    D = B.make_case(c)
    dev = Dev(c, D)
    fw = fwd_reference(c)
    N, R, Cc = c.N, c.R, c.C
    assert c.sizes()['out'] == N * R * Cc
    worst = 0.0
    for with_lo in ((1, 0) if c.y_f32 else (0,)):
        hi = Buf((N, R, Cc), torch.bfloat16)
        lo = Buf((N, R, Cc), torch.bfloat16) if with_lo else None
        mask = Buf((c.sizes()['mask'],), torch.uint8) if c.p > 0 else None
        q = Buf((N, R, Cc), torch.uint8) if c.q_scale else None
        qc = Buf((1,), torch.int64, torch.tensor([7])) if c.q_scale else None
        d = dev.desc(L, mask=mask, mean=None, invstd=None, mean2=None, invstd2=None, q_clipped=addr(qc))
        args = (c.R, c.pad_l, c.pad_r, c.pad_mode, L.stream_ptr())
        if q is None:
            run(L, L.lib.w2l_bn_act_fwd(ctypes.byref(d), p(L, hi), p(L, lo), *args))
        else:
            run(L, L.lib.w2l_bn_act_fwd_q(ctypes.byref(d), p(L, hi), p(L, lo), p(L, q), c.q_scale, *args))
        what = f'bn_act_fwd {c.name} lo={with_lo}'
        worst = max(worst, check_forward(c, fw, hi, lo, q, mask, 7, qc, what))
        if q is not None:                               # a second call ADDS to the counter
            first = int(qc.np()[0])
            run(L, L.lib.w2l_bn_act_fwd_q(ctypes.byref(d), p(L, hi), p(L, lo), p(L, q), c.q_scale, *args))
            assert int(qc.np()[0]) - first == first - 7, f'{what}: the second call adds the same count'
        assert guards(hi, lo, mask, q, qc, *dev.inputs()), what
    record('bn_act_fwd', c.name, worst)


def test_bn_act_fwd_offset_dev(L):
    """a device word of 5 added to offset = 1 gives the bytes of offset = 6"""
    c = next(x for x in B.FWD_ONLY if x.name == 'c8')
    D = B.make_case(c)
    dev = Dev(c, D)
    word = Buf((1,), torch.int64, torch.tensor([5]))
    hi, mask = Buf((c.N, c.R, c.C), torch.bfloat16), Buf((c.sizes()['mask'],), torch.uint8)
    d = dev.desc(L, mask=mask, offset=1, offset_dev=addr(word))
    run(L, L.lib.w2l_bn_act_fwd(ctypes.byref(d), p(L, hi), None, c.R, c.pad_l, c.pad_r, c.pad_mode, L.stream_ptr()))
    fw = B.fwd_ref_of(c, D, offset=6)
    assert fw['mask_written'].all() and np.array_equal(mask.np(), fw['mask']) and not np.array_equal(fw['mask'], fwd_reference(c)['mask'])
    r = ratio(hi.np(), fw['a'].v, fw['a'].bound(B.R_BF16))
    assert r <= 1 and guards(hi, mask, word) and int(word.np()[0]) == 5
    record('bn_act_fwd', 'offset_dev', r)


# ================================================================================================================================
# forward with the finalize folded in: w2l_bn_act_fwd_fin
# ================================================================================================================================

class FinRec:
    """one w2l_bnfin_t with its buffers and its reference; the statistics rows are those of the branch's own y, gamma / beta
    chosen so that the published scale / shift come out near the case's"""

    def __init__(self, L, y, rows, scale, shift, running, stats, null_partial=False):
        Cc = y.shape[-1]
        x = y.reshape(-1, Cc).astype(np.float64)
        M = x.shape[0]
        cuts = np.linspace(0, M, rows + 1).astype(int)
        pr = np.stack([np.stack([x[a:b].sum(0), (x[a:b] ** 2).sum(0)]) for a, b in zip(cuts[:-1], cuts[1:])]).astype(np.float32)
        istd = 1 / np.sqrt(x.var(0) + EPS)
        ga = (scale / istd).astype(np.float32)
        be = (shift + x.mean(0) * scale).astype(np.float32)
        rng = np.random.default_rng(rows)
        rm = rng.standard_normal(Cc).astype(np.float32) if running else None
        rv = (rng.random(Cc) + 0.5).astype(np.float32) if running else None
        self.ref = None if null_partial else B.bn_finalize_ref(pr, Cc, M, ga, be, EPS, MOM, rm, rv)
        self.P, self.Ga, self.Be, self.Rm, self.Rv = (None if null_partial else up(pr)), up(ga), up(be), up(rm), up(rv)
        self.rm0, self.rv0 = rm, rv
        self.out = {k: Buf((Cc,)) for k in (('mean', 'invstd') if stats else ()) + ('scale', 'shift')}
        self.rec = L.BnFin(partial=addr(self.P), rows=rows, count=M, gamma=addr(self.Ga), beta=addr(self.Be), eps=EPS, momentum=MOM,
                           running_mean=addr(self.Rm), running_var=addr(self.Rv), mean=addr(self.out.get('mean')),
                           invstd=addr(self.out.get('invstd')), scale=addr(self.out['scale']), shift=addr(self.out['shift']))

    def check(self, what):
        """published statistics against bn_finalize_ref; returns (worst ratio, published scale, published shift)"""
        if self.ref is None:                            # partial = NULL: nothing is published, nothing updated
            assert all(bool(torch.isnan(b.flat).all()) for b in self.out.values()), what
            assert self.Rm is None or (np.array_equal(self.Rm.np(), self.rm0) and np.array_equal(self.Rv.np(), self.rv0))
            return 0.0, None, None
        got = {k: b.np() for k, b in self.out.items()}
        if self.Rm is not None:
            got.update(running_mean=self.Rm.np(), running_var=self.Rv.np())
        worst = 0.0
        for k, v in got.items():
            r = ratio(v, self.ref[k].v, self.ref[k].bound())
            assert r <= 1, f'{what} {k}: error / bound = {r}'
            worst = max(worst, r)
        assert guards(self.P, self.Ga, self.Be, self.Rm, self.Rv, *self.out.values()), what
        return worst, got['scale'], got['shift']


def fwd_fin_once(L, c, rows1, rows2, null2, running, stats):
    D = B.make_case(c)
    dev = Dev(c, D)
    f1 = FinRec(L, D['y'], rows1, D['scale'], D['shift'], running, stats)
    f2 = FinRec(L, D['y2'], rows2, D['scale2'], D['shift2'], running, stats, null_partial=null2) if c.res else None
    N, R, Cc = c.N, c.R, c.C
    hi = Buf((N, R, Cc), torch.bfloat16)
    mask = Buf((c.sizes()['mask'],), torch.uint8) if c.p > 0 else None
    q = Buf((N, R, Cc), torch.uint8) if c.q_scale else None
    qc = Buf((1,), torch.int64, torch.tensor([7])) if c.q_scale else None
    # the descriptor's own scale / shift are ignored for a branch with statistics rows
    d = dev.desc(L, mask=mask, scale=None, shift=None, mean=None, invstd=None, mean2=None, invstd2=None, q_clipped=addr(qc),
                 **({} if (c.res and null2) else dict(scale2=None, shift2=None)))
    run(L, L.lib.w2l_bn_act_fwd_fin(ctypes.byref(d), ctypes.byref(f1.rec), ctypes.byref(f2.rec) if f2 else None, p(L, hi), p(L, q),
                                    c.q_scale or 1.0, R, c.pad_l, c.pad_r, c.pad_mode, L.stream_ptr()))
    what = f'bn_act_fwd_fin {c.name} rows={rows1},{rows2} null2={null2}'
    w1, sc1, sh1 = f1.check(what + ' branch 1')
    w2, sc2, sh2 = f2.check(what + ' branch 2') if f2 else (0.0, None, None)
    if c.res and null2:
        sc2, sh2 = D['scale2'], D['shift2']
    # the activation against the reference fed with the PUBLISHED scale / shift
    fw = B.bn_act_fwd_ref(N, c.T, Cc, D['y'], sc1, sh1, D['y2'], sc2, sh2, act=c.act, p=c.p, seed=D['seed'], offset=D['offset'],
                          lens=D['lens'], out_rows=R, pad_l=c.pad_l, pad_r=c.pad_r, pad_mode=c.pad_mode, q_scale=c.q_scale or None)
    wa = check_forward(c, fw, hi, None, q, mask, 7, qc, what)
    assert guards(hi, mask, q, qc, *dev.inputs()), what
    return max(w1, w2), wa


def test_bn_act_fwd_fin_small(L):
    c = B.FWD_FIN_SMALL
    ws = wa = 0.0
    for rows1, rows2, null2, running, stats in ((3, 8, False, True, True), (8, 3, True, False, False), (1, 8, False, True, False)):
        s, a = fwd_fin_once(L, c, rows1, rows2, null2, running, stats)
        ws, wa = max(ws, s), max(wa, a)
    record('bn_act_fwd_fin', f'{c.name} statistics', ws)
    record('bn_act_fwd_fin', f'{c.name} activation', wa)


def test_bn_act_fwd_fin_two_batches(L):
    c = B.FWD_FIN_BIG
    s, a = fwd_fin_once(L, c, 3, 0, False, True, True)
    record('bn_act_fwd_fin', f'{c.name} statistics', s)
    record('bn_act_fwd_fin', f'{c.name} activation', a)


# ================================================================================================================================
# backward, general path: reduce + finalize, apply, apply_amax, apply_fin
# ================================================================================================================================

@functools.lru_cache(maxsize=2)
def bwd_reference(c):
    """own sums, depth 0 on top of the terms' (redepth adds each kernel tree's); dy frames in the halo = 0 layout"""
    return B.bwd_ref_of(c, B.make_case(c), sum_depth=0)


def apply_variants(c):
    """(halo, halo2, dy_lo, dy2) of the dy launches of a case: halos 0 / 1 / 13 with halo2 another, lo given and not, dy2 NULL with
    a residual branch present"""
    v = [(0, 1, 1, 1), (13, 0, 0, 1), (1, 13, 1, 0)]
    return [(1, 13, 0, 1)] if B.is_big(c) else v


def dy_buffers(c, halo, halo2, with_lo, with_dy2):
    s = c.sizes(halo, halo2)
    rows, rows2 = halo + c.N * (c.T + halo), halo2 + c.N * (c.T + halo2)
    assert s['dy'] == rows * c.C and s['dy2'] == rows2 * c.C
    hi = Buf((rows, c.C), torch.bfloat16)
    lo = Buf((rows, c.C), torch.bfloat16) if with_lo else None
    two = bool(c.res) and with_dy2
    hi2 = Buf((rows2, c.C), torch.bfloat16) if two else None
    lo2 = Buf((rows2, c.C), torch.bfloat16) if two and with_lo else None
    return hi, lo, hi2, lo2


def check_dy(c, ref, bufs, halo, halo2, what):
    hi, lo, hi2, lo2 = bufs
    r = dy_ratio(hi, lo, ref['dy'], c.N, c.T, halo)
    if hi2 is not None:
        r = max(r, dy_ratio(hi2, lo2, ref['dy2'], c.N, c.T, halo2))
    assert r <= 1, f'{what}: dy error / bound = {r}'
    assert guards(*bufs), what
    return r


@pytest.mark.parametrize('c', B.GENERAL + [B.BIG_APPLY], ids=lambda c: c.name)
def test_bn_bwd_general(L, c):
    D = B.make_case(c)
    dev = Dev(c, D)
    N, T, Cc = c.N, c.T, c.C
    ncomp = 4 if c.res else 2
    nb = L.lib.w2l_bn_bwd_blocks(N, T, Cc)
    assert nb == B.bwd_blocks(N, T, Cc) and c.sizes()['partial'] == nb * ncomp * Cc
    g1, g2 = dev.srcs(L)
    refs = (ctypes.byref(g1), ctypes.byref(g2) if g2 else None)
    d = dev.desc(L)
    assert L.lib.w2l_bn_bwd_fast_ok(ctypes.byref(d), *refs) == int(not c.y_f32 and not c.res and not c.g_f32 and not c.two_src
                                                                   and bool(c.bn1))
    base = bwd_reference(c)
    sp = L.stream_ptr()
    # ---- reduce + finalize: the sums
    partial, sums = Buf((nb, ncomp, Cc)), Buf((4, Cc))
    run(L, L.lib.w2l_bn_act_bwd_reduce(ctypes.byref(d), *refs, p(L, partial), sp))
    run(L, L.lib.w2l_bn_bwd_finalize(p(L, partial), nb, Cc, ncomp, p(L, sums), sp))
    ref = B.redepth(base, B.general_sum_depth(N, T, Cc, 'finalize'))
    rs = ratio(sums.np()[:ncomp], ref['sums'].v, ref['sums'].bound())
    assert rs <= 1, f'bn_bwd reduce + finalize {c.name}: sums error / bound = {rs}'
    assert np.isnan(sums.np()[ncomp:]).all() and not np.isnan(partial.np()).any() and guards(partial, sums, *dev.inputs())
    record('bn_bwd_reduce+finalize', c.name, rs)
    # ---- apply / apply_amax read the DEVICE's sums: an exact input of their reference
    worst = 0.0
    if not B.is_big(c) or c is B.BIG_APPLY:
        given = B.bwd_ref_of(c, D, sums=sums.np()[:ncomp].astype(np.float64), sum_depth=0)
        for i, (halo, halo2, with_lo, with_dy2) in enumerate(apply_variants(c)):
            if c is B.BIG_APPLY:
                halo = 40
            for use_amax in (0, 1):
                bufs = dy_buffers(c, halo, halo2, with_lo, with_dy2)
                amax = Buf((2, B.AMAX_SLOTS), init=torch.zeros(2, B.AMAX_SLOTS)) if use_amax else None
                sums_arg = p(L, sums) if (c.bn1 or c.res == 1) else None
                a = (ctypes.byref(d), *refs, sums_arg, p(L, bufs[0]), p(L, bufs[1]), halo, p(L, bufs[2]), p(L, bufs[3]), halo2)
                if use_amax:
                    run(L, L.lib.w2l_bn_act_bwd_apply_amax(*a, p(L, amax), sp))
                    amax_check(amax, [given['dy'], given['dy2'] if bufs[2] is not None else None], c.name)
                    assert guards(amax)
                else:
                    run(L, L.lib.w2l_bn_act_bwd_apply(*a, sp))
                worst = max(worst, check_dy(c, given, bufs, halo, halo2, f'bn_act_bwd_apply{"_amax" if use_amax else ""} {c.name} '
                                            f'halo={halo},{halo2} lo={with_lo} dy2={with_dy2}'))
        record('bn_act_bwd_apply(_amax)', c.name, worst)
    # ---- apply_fin: the sums are internal, their Tr is carried into dy
    if c is not B.BIG_APPLY:
        ref = B.redepth(base, B.general_sum_depth(N, T, Cc, 'apply_fin'))
        worst = 0.0
        for halo, halo2, with_lo, with_dy2 in apply_variants(c):
            bufs = dy_buffers(c, halo, halo2, with_lo, with_dy2)
            sums2 = Buf((4, Cc))
            amax = Buf((2, B.AMAX_SLOTS), init=torch.zeros(2, B.AMAX_SLOTS)) if halo == 1 or B.is_big(c) else None
            run(L, L.lib.w2l_bn_act_bwd_apply_fin(ctypes.byref(d), *refs, p(L, partial), nb, p(L, sums2), p(L, bufs[0]), p(L, bufs[1]), halo,
                                                  p(L, bufs[2]), p(L, bufs[3]), halo2, p(L, amax), sp))
            r = ratio(sums2.np()[:ncomp], ref['sums'].v, ref['sums'].bound())
            assert r <= 1 and np.isnan(sums2.np()[ncomp:]).all() and guards(sums2), f'bn_act_bwd_apply_fin {c.name}: sums error / bound = {r}'
            worst = max(worst, r, check_dy(c, ref, bufs, halo, halo2, f'bn_act_bwd_apply_fin {c.name} halo={halo},{halo2} lo={with_lo}'))
            if amax is not None:
                amax_check(amax, [ref['dy'], ref['dy2'] if bufs[2] is not None else None], c.name)
        record('bn_act_bwd_apply_fin', c.name, worst)
    assert guards(*dev.inputs())


@pytest.mark.parametrize('nblocks', [1, 9, 57, 64, 65])
def test_bwd_finalize_rows(L, nblocks):
    """w2l_bn_bwd_finalize is a column sum of whatever rows it is given: d = nblocks"""
    rng = np.random.default_rng(nblocks)
    worst = 0.0
    for ncomp, Cc in ((2, 64), (4, 72)):
        pr = rng.standard_normal((nblocks, ncomp * Cc)).astype(np.float32)
        P_, sums = up(pr), Buf((4, Cc))
        run(L, L.lib.w2l_bn_bwd_finalize(p(L, P_), nblocks, Cc, ncomp, p(L, sums), L.stream_ptr()))
        ref = Tr(pr.astype(np.float64).sum(0), np.abs(pr.astype(np.float64)).sum(0), nblocks)
        r = ratio(sums.np().reshape(-1)[:ncomp * Cc], ref.v, ref.bound())
        assert r <= 1 and np.isnan(sums.np().reshape(-1)[ncomp * Cc:]).all() and guards(P_, sums), (nblocks, ncomp, r)
        worst = max(worst, r)
    record('bn_bwd_finalize', f'nblocks={nblocks}', worst)


@pytest.mark.parametrize('nblocks', [1, 4, 13, 16, 17, 29])
def test_apply_fin_rows(L, nblocks):
    """apply_fin's prologue sums whatever partial rows it is given (the 16-step loop and its 4-step tail, per wave): random rows,
    their exact column sums (d = nblocks) carried into dy"""
    worst = 0.0
    for c in (B.GENERAL[0], B.GENERAL[2]):
        D = B.make_case(c)
        dev = Dev(c, D)
        ncomp = 4 if c.res else 2
        rng = np.random.default_rng(nblocks)
        pr = rng.standard_normal((nblocks, ncomp, c.C)).astype(np.float32)
        if ncomp == 4:
            pr[:, 2] = pr[:, 0]
        s64 = Tr(pr.astype(np.float64).sum(0), np.abs(pr.astype(np.float64)).sum(0), nblocks)
        ref = B.bwd_ref_of(c, D, sums=s64)
        g1, g2 = dev.srcs(L)
        halo, halo2 = 13, 1                             # 13 * (N + 1) = 52 halo rows: no multiple of 32
        bufs = dy_buffers(c, halo, halo2, 0, 1)
        P_, sums = up(pr), Buf((4, c.C))
        d = dev.desc(L)
        run(L, L.lib.w2l_bn_act_bwd_apply_fin(ctypes.byref(d), ctypes.byref(g1), ctypes.byref(g2) if g2 else None, p(L, P_), nblocks, p(L, sums),
                                              p(L, bufs[0]), None, halo, p(L, bufs[2]), None, halo2, None, L.stream_ptr()))
        r = ratio(sums.np()[:ncomp], s64.v, s64.bound())
        assert r <= 1 and guards(P_, sums, *dev.inputs()), f'apply_fin nblocks={nblocks} {c.name}: sums error / bound = {r}'
        worst = max(worst, r, check_dy(c, ref, bufs, halo, halo2, f'apply_fin nblocks={nblocks} {c.name}'))
    record('bn_act_bwd_apply_fin', f'nblocks={nblocks}', worst)


# ================================================================================================================================
# backward, the slot chain: reduce_slots + apply_slots (one-shot U = 1 / 2 / 4 and the looped kernels)
# ================================================================================================================================

SLOT_RUNS = {'loop_threshold': (1,), 'loop_t8': (8,), 'oneshot_t7': (64,), 'oneshot_below': (8,)}


@pytest.mark.parametrize('c', B.SLOTS + B.LOOPED, ids=lambda c: c.name)
def test_bn_bwd_slots(L, c):
    D = B.make_case(c)
    dev = Dev(c, D)
    N, T, Cc = c.N, c.T, c.C
    g1, _ = dev.srcs(L)
    d = dev.desc(L)
    assert L.lib.w2l_bn_bwd_fast_ok(ctypes.byref(d), ctypes.byref(g1), None) == 1
    base = bwd_reference(c)
    sp = L.stream_ptr()
    worst_s = worst_d = 0.0
    for i, slots in enumerate(SLOT_RUNS.get(c.name, (1, 8, 64))):
        for use_amax in ((int(c.name in ('loop_t8', 'oneshot_t7')),) if B.is_big(c) else (0, 1)):
            halo = (0, 13, 1)[i % 3] if not B.is_big(c) else 7
            ref = B.redepth(base, B.slots_sum_depth(N, T, Cc, slots, slots))
            partial = Buf((slots, 2, Cc), init=torch.zeros(slots, 2, Cc))
            sums = Buf((4, Cc))
            hi, _, _, _ = bufs = dy_buffers(c, halo, 0, 0, 0)
            amax = Buf((2, B.AMAX_SLOTS), init=torch.zeros(2, B.AMAX_SLOTS)) if use_amax else None
            run(L, L.lib.w2l_bn_act_bwd_reduce_slots(ctypes.byref(d), ctypes.byref(g1), p(L, partial), slots, sp))
            run(L, L.lib.w2l_bn_act_bwd_apply_slots(ctypes.byref(d), ctypes.byref(g1), p(L, partial), slots, p(L, sums), p(L, hi), halo,
                                                    p(L, amax), sp))
            what = f'bn_bwd slots {c.name} slots={slots} halo={halo} amax={use_amax}'
            r = ratio(sums.np()[:2], ref['sums'].v, ref['sums'].bound())
            assert r <= 1, f'{what}: sums error / bound = {r}'
            assert np.isnan(sums.np()[2:]).all() and guards(partial, sums)
            worst_s = max(worst_s, r)
            worst_d = max(worst_d, check_dy(c, ref, bufs, halo, 0, what))
            if amax is not None:
                amax_check(amax, [ref['dy'], None], what)
                assert guards(amax)
    assert guards(*dev.inputs())
    record('bn_act_bwd_reduce_slots', c.name, worst_s)
    record('bn_act_bwd_apply_slots', c.name, worst_d)


# ================================================================================================================================
# e4m3 quantisation
# ================================================================================================================================

def test_quantize(L):
    """w2l_quantize_e4m3 with a power-of-two scale: src * scale is exact, the codes are e4m3_rne_sat's"""
    rng = np.random.default_rng(2)
    n = 8 * (4096 * 256 + 256)                          # n / 8 above 4096 x 256 groups: the grid-stride loop's second round
    for src_f32, count, scale in ((0, n, 4.0), (1, 8 * 1000, 0.5), (0, 8, 64.0)):
        x = (rng.standard_normal(count) * 60).astype(np.float32)
        x[:8] = [0.0, -0.0, 448.0, -500.0, 2.0 ** -9, 2.0 ** -10, 17.0, -19.0]
        x = x if src_f32 else B.bf16_to_f32(B.bf16_rne(x))
        src = up(x, torch.float32 if src_f32 else torch.bfloat16)
        dst = Buf((count,), torch.uint8)
        run(L, L.lib.w2l_quantize_e4m3(p(L, src), src_f32, count, scale, p(L, dst), L.stream_ptr()))
        want = B.e4m3_rne_sat(x.astype(np.float64) * scale)
        got = dst.np()
        assert np.array_equal(got & 0x7F, want & 0x7F) and np.array_equal((got >> 7)[want & 0x7F != 0], (want >> 7)[want & 0x7F != 0])
        assert guards(src, dst)


AMAXES = [224.0, 112.0, 448.0, 7.0, 1.75, 224.0 * 2.0 ** -20]


def bf16_neighbours(a):
    b = int(B.bf16_rne(np.array([a], dtype=np.float32))[0])
    return [float(B.bf16_to_f32(np.array([b + k], dtype=np.uint16))[0]) for k in (-1, 0, 1)]


def test_quantize_dyn(L):
    """where 224 / amax is an exact power of two floor(log2(.)) must not land a binade low; inv_scale EQUALS the reference's and
    the codes are e4m3(src * s) exactly (src bf16, s a power of two)"""
    rng = np.random.default_rng(3)
    n_big = 8 * (4096 * 256 + 256)
    runs = [(a, j) for a0 in AMAXES for j, a in enumerate(bf16_neighbours(a0))] + [(0.0, 0)]
    for i, (a, j) in enumerate(runs):
        count = n_big if i == 1 else 8 * 640
        slots = (rng.random(B.AMAX_SLOTS) * a * 0.9).astype(np.float32)
        slots[(7 * i + 3 * j) % B.AMAX_SLOTS] = a
        s, inv = B.quantize_dyn_ref(slots)
        x = B.bf16_to_f32(B.bf16_rne(((rng.random(count) * 2.2 - 1.1) * max(a, 1.0)).astype(np.float32)))
        src, am = up(x, torch.bfloat16), up(slots)
        dst, iv = Buf((count,), torch.uint8), Buf((1,))
        run(L, L.lib.w2l_quantize_e4m3_dyn(p(L, src), count, p(L, am), p(L, dst), p(L, iv), L.stream_ptr()))
        assert float(iv.np()[0]) == inv, f'quantize_e4m3_dyn amax={a!r}: inv_scale {float(iv.np()[0])!r}, reference {inv!r}'
        want = B.e4m3_rne_sat(x.astype(np.float64) * s)
        got = dst.np()
        nz = want & 0x7F != 0
        assert np.array_equal(got & 0x7F, want & 0x7F) and np.array_equal((got >> 7)[nz], (want >> 7)[nz]), f'amax={a!r}'
        assert guards(src, am, dst, iv)


# ================================================================================================================================
# argument checks
# ================================================================================================================================

def test_bn_argument_checks(L):
    """each set is refused by a W2L_CHECK_ARG in front of the launch: nonzero return, its message, the outputs untouched"""
    c = B.SLOTS[1]                                      # bf16, one branch, one source, C = 128, zero padding 2 / 3
    D = B.make_case(c)
    dev = Dev(c, D)
    N, T, Cc, R = c.N, c.T, c.C, c.R
    out = Buf((N, R + 2 * T, Cc), torch.bfloat16)
    mask = Buf((c.sizes()['mask'],), torch.uint8)
    fl = Buf((64, 4, Cc))
    g1, _ = dev.srcs(L)
    sp = L.stream_ptr()
    D_ = lambda **kw: ctypes.byref(dev.desc(L, **kw))
    G_ = lambda **kw: ctypes.byref(L.GradSrc(**{**dict(dxp=addr(dev.g[0]), f32=0, pad_l=c.pad_l, pad_r=c.pad_r, pad_mode=0, rows=R), **kw}))
    fin = L.BnFin(partial=addr(fl), rows=3, count=N * T, eps=EPS, momentum=MOM, scale=addr(fl), shift=addr(fl))
    fwd = lambda d, rows=R, pl=c.pad_l, pr=c.pad_r, pm=0: L.lib.w2l_bn_act_fwd(d, p(L, out), None, rows, pl, pr, pm, sp)
    ffin = lambda d: L.lib.w2l_bn_act_fwd_fin(d, ctypes.byref(fin), None, p(L, out), None, 1.0, R, c.pad_l, c.pad_r, 0, sp)
    red = lambda d, g, g2=None: L.lib.w2l_bn_act_bwd_reduce(d, g, g2, p(L, fl), sp)
    app = lambda d, g, g2=None: L.lib.w2l_bn_act_bwd_apply(d, g, g2, p(L, fl), p(L, out), None, 0, None, None, 0, sp)
    afin = lambda d, g: L.lib.w2l_bn_act_bwd_apply_fin(d, g, None, p(L, fl), 4, p(L, fl), p(L, out), None, 0, None, None, 0, None, sp)
    rsl = lambda d, g, s: L.lib.w2l_bn_act_bwd_reduce_slots(d, g, p(L, fl), s, sp)
    asl = lambda d, g: L.lib.w2l_bn_act_bwd_apply_slots(d, g, p(L, fl), 4, p(L, fl), p(L, out), 0, None, sp)
    calls = {
        'fwd C%8': (lambda: fwd(D_(C=Cc + 4)), 'bn_act_fwd: bad N/T/C'),
        'fwd C>2048': (lambda: fwd(D_(C=2056)), 'bn_act_fwd: bad N/T/C'),
        'fwd p=1': (lambda: fwd(D_(drop_p=1.0, mask=mask)), 'bn_act_fwd: dropout p'),
        'fwd dropout without a mask': (lambda: fwd(D_(drop_p=0.3, mask=None)), 'bn_act_fwd: dropout needs a mask'),
        'fwd scale without shift': (lambda: fwd(D_(shift=None)), 'bn_act_fwd: scale/shift'),
        'fwd reflect pad >= T': (lambda: fwd(D_(), rows=R + 2 * T, pl=T, pr=1, pm=1), 'bn_act_fwd: reflect pad'),
        'fwd out_rows too small': (lambda: fwd(D_(), rows=c.pad_l + T + c.pad_r - 1), 'bn_act_fwd: bad output geometry'),
        'fwd q_scale 0': (lambda: L.lib.w2l_bn_act_fwd_q(D_(), p(L, out), None, p(L, out), 0.0, R, c.pad_l, c.pad_r, 0, sp),
                          'bn_act_fwd: the e4m3 copy'),
        'fwd per_utt >= 2^24': (lambda: fwd(D_(C=2048), rows=65536), 'bn_act_fwd: more than 2^24'),
        'fwd_fin fp32 y': (lambda: ffin(D_(y_f32=1)), 'bn_act_fwd_fin: bf16 y only'),
        'fwd_fin C%64': (lambda: ffin(D_(C=72)), 'bn_act_fwd_fin: C=72'),
        'fwd_fin record count': (lambda: L.lib.w2l_bn_act_fwd_fin(D_(), ctypes.byref(fin), ctypes.byref(fin), p(L, out), None, 1.0, R, c.pad_l,
                                                                  c.pad_r, 0, sp), 'bn_act_fwd_fin: one finalize record'),
        'reduce C%64': (lambda: red(D_(C=72), G_()), 'bn_act_bwd_reduce: C=72'),
        'reduce too few rows': (lambda: red(D_(), G_(rows=R - c.tail - 1)), 'bn_act_bwd_reduce: gradient source has too few rows'),
        'reduce mixed dtypes': (lambda: red(D_(), G_(), G_(f32=1)), 'bn_act_bwd_reduce: gradient sources must share'),
        'apply too few rows': (lambda: app(D_(), G_(), G_(rows=T)), 'bn_act_bwd_apply: gradient source has too few rows'),
        'apply without sums': (lambda: L.lib.w2l_bn_act_bwd_apply(D_(), G_(), None, None, p(L, out), None, 0, None, None, 0, sp),
                               'bn_act_bwd_apply: BatchNorm backward needs'),
        'apply negative halo': (lambda: L.lib.w2l_bn_act_bwd_apply(D_(), G_(), None, p(L, fl), p(L, out), None, -1, None, None, 0, sp),
                                'bn_act_bwd_apply: negative halo'),
        'apply_fin C%64': (lambda: afin(D_(C=72), G_()), 'bn_act_bwd_apply_fin: C=72'),
        'apply_fin no rows': (lambda: L.lib.w2l_bn_act_bwd_apply_fin(D_(), G_(), None, p(L, fl), 0, p(L, fl), p(L, out), None, 0, None, None, 0,
                                                                     None, sp), 'bn_act_bwd_apply_fin: null pointer'),
        'reduce_slots 0': (lambda: rsl(D_(), G_(), 0), 'bn_act_bwd_reduce_slots: null pointer / slots'),
        'reduce_slots 65': (lambda: rsl(D_(), G_(), 65), 'bn_act_bwd_reduce_slots: null pointer / slots'),
        'reduce_slots fp32 y': (lambda: rsl(D_(y_f32=1), G_(), 4), 'bn_act_bwd_reduce_slots: bf16 y and gradient'),
        'reduce_slots fp32 gradient': (lambda: rsl(D_(), G_(f32=1), 4), 'bn_act_bwd_reduce_slots: bf16 y and gradient'),
        'reduce_slots residual': (lambda: rsl(D_(y2=addr(dev.y)), G_(), 4), 'bn_act_bwd_reduce_slots: bf16 y and gradient'),
        'reduce_slots no BatchNorm': (lambda: rsl(D_(scale=None, shift=None), G_(), 4), 'bn_act_bwd_reduce_slots: bf16 y and gradient'),
        'apply_slots C%64': (lambda: asl(D_(C=72), G_()), 'bn_act_bwd_apply_slots: bf16 y and gradient'),
        'apply_slots too few rows': (lambda: asl(D_(), G_(rows=T)), 'bn_act_bwd_apply_slots: gradient source has too few rows'),
        'finalize null output': (lambda: L.lib.w2l_bn_finalize(p(L, fl), 4, Cc, N * T, None, None, EPS, MOM, None, None, None, None, None,
                                                               p(L, out), sp), 'bn_finalize: null output'),
        'finalize eval without running': (lambda: L.lib.w2l_bn_finalize(None, 0, Cc, 0, None, None, EPS, MOM, None, None, None, None, p(L, fl),
                                                                        p(L, fl), sp), 'bn_finalize: eval mode'),
        'finalize no tiles': (lambda: L.lib.w2l_bn_finalize(p(L, fl), 0, Cc, N * T, None, None, EPS, MOM, None, None, None, None, p(L, fl),
                                                            p(L, fl), sp), 'bn_finalize: bad tile count'),
        'bwd_finalize ncomp': (lambda: L.lib.w2l_bn_bwd_finalize(p(L, fl), 4, Cc, 3, p(L, fl), sp), 'bn_bwd_finalize: bad arguments'),
        'quantize n%8': (lambda: L.lib.w2l_quantize_e4m3(p(L, out), 0, 12, 1.0, p(L, mask), sp), 'quantize_e4m3: bad arguments'),
        'quantize_dyn n%8': (lambda: L.lib.w2l_quantize_e4m3_dyn(p(L, out), 12, p(L, fl), p(L, mask), p(L, fl), sp),
                             'quantize_e4m3_dyn: bad arguments'),
    }
    for name, (call, msg) in calls.items():
        assert call() != 0, name
        assert last_error(L).startswith(msg), (name, last_error(L))
    torch.cuda.synchronize()
    assert bool(torch.isnan(out.flat).all()) and bool(torch.isnan(fl.flat).all()) and bool((mask.flat == 0xA5).all())
    assert guards(*dev.inputs())
    assert L.lib.w2l_bn_bwd_blocks(0, 5, 64) == 0 and L.lib.w2l_bn_bwd_blocks(3, 5, 32) == 0
