"""Float64 references of the e4m3 kernels (csrc/conv_wgrad_fp8.hip: w2l_conv1d_wgrad_fp8; csrc/conv_igemm.hip, F8:
w2l_conv1d_igemm_fp8 and the fused inference epilogue w2l_conv1d_igemm_bnact_fp8) -- plain NumPy, nothing of the engine's
Python -- with the cases, the two operand families, the planted defects and the forced plans that tests/test_cpu_fp8_refs.py
(no GPU) and tests/test_gpu_fp8_direct.py share.

Two operand families.

  exact       e4m3 codes of integers drawn from [-4, 4] per element; descale, *descale_dev powers of two; the accumulate operand
              and the bias multiples of 2^-4.  A product of two e4m3 values is exact in fp32 (4 + 4 significand bits), here an
              integer of magnitude <= 16.  One MFMA (v_mfma_scale_f32_16x16x128_f8f6f4) sums 128 of them: <= 128 x 16 = 2^11.
              A whole reduction of K products is an integer of magnitude <= 16 K < 2^24 (exact_units() is the figure per case and
              the CPU test asserts it below 2^24; at the cases here it stays below 2^16), so EVERY partial sum, in whatever order
              -- MFMA chains, K steps, atomics in arrival order -- is an integer fp32 holds exactly.  The factors are powers of
              two and the added operands multiples of the result's unit, so nothing rounds anywhere: the device result must equal
              the reference BIT FOR BIT (np.array_equal on the fp32 bits).  A mismatch is an indexing defect, never rounding.
  full range  codes uniform over the 254 finite e4m3 bytes (subnormals, both zeros and +-448), factors that are no powers of
              two.  |got - v| <= (M K + c) u A per element: u = 2^-24, v and A = |descale| sum |a||b| from float64, K the
              products of the element, c the roundings outside the dot product, counted from the code (wgrad_c(), conv_c()),
              M = F8_DOT_MARGIN, the one number that is measured, not derived.

The planted defects are mistakes in the kernels' index arithmetic that a whole-tensor criterion cannot see; the CPU test
proves that each changes a bit of the exact family wherever it applies and lies outside the full-range bound on at least one
case."""
import dataclasses

import numpy as np

import conv_refs as C
from bn_refs import E4M3, e4m3_bound, e4m3_rne_sat  # noqa: F401  (re-exported)
from kernel_refs import Tr, U, bf16_rne, bf16_to_f32, f32  # noqa: F401  (re-exported)

# the factor on the dot product's share of the bound: 1 would mean that the matrix unit's accumulation of K exact products obeys
# K u A against float64, as the bf16 unit does (0.0106 of it).  v_mfma_scale_f32_16x16x128_f8f6f4 does not: measured on an MI355X
# (tests/test_gpu_fp8_direct.py prints error / bound per family, at this margin and at margin 1), the worst error / ((K + c) u A)
# is 14.56 on the weight gradient (case W5, K = 150; 5.93 at K = 256, 2.70 at K = 390, 0.44 at K = 1285) and 6.45 on the
# convolution (case F2, K = 256; 1.53 at K = 640, 0.59 at K = 1152) while the exact family is bit-equal on every plan and block
# shape.  The error is about 600 .. 2200 u A whatever K is: it belongs to the 128-term sum inside one instruction and does not grow with the number of
# instructions, so the K u A form is loosest at a long reduction.  The margin is the smallest power of two that is at least twice
# the measured worst; tests/test_cpu_fp8_refs.py proves that every planted defect still lies outside the bound at it
F8_DOT_MARGIN = 32.0

NAN8 = 0x7F                   # the e4m3 NaN code: what fills every byte the contract does not let a kernel read
BT = 128                      # frames of a K step of the weight gradient = the reduction length of one MFMA
TILE = 128                    # channels of a co / ci tile

FAMILIES = ('exact', 'full')


def codes_exact(rng, shape):
    """e4m3 codes of integers drawn from [-4, 4]"""
    c = e4m3_rne_sat(rng.integers(-4, 5, size=shape).astype(np.float64))
    assert np.array_equal(E4M3[c], np.rint(E4M3[c])) and np.abs(E4M3[c]).max() <= 4
    return c


_FINITE = np.array([b for b in range(256) if (b & 0x7F) != 0x7F], dtype=np.uint8)


def codes_full(rng, shape):
    """codes uniform over the 254 finite e4m3 bytes"""
    return _FINITE[rng.integers(0, len(_FINITE), size=shape)]


def codes(family, rng, shape):
    return codes_exact(rng, shape) if family == 'exact' else codes_full(rng, shape)


# the factors of the two families: (descale, *descale_dev).  Exact: powers of two.  Full range: neither is one
FACTORS = {'exact': (2.0 ** -3, 2.0 ** -2), 'full': (f32(1.0 / 48.0), f32(0.0123))}
EXACT_UNIT = 2.0 ** -5        # the smallest unit an exact-family result is a multiple of: descale x *descale_dev


# ================================================================================================================================
# A. the weight gradient
#
#   dw[k][co][ci] = descale (*descale_dev) sum_{n, t < Tout} dyq[n][t][co] xq[n][t + k dil][ci]     (+ dw0 with accumulate = 1)
#
# The kernel walks each utterance in tsteps = ceil(Tout / 128) steps of 128 frames: it reads dy rows [0, 128 tsteps) of every
# utterance -- rows from Tout on must be ZERO -- and the x rows beneath them (clamped onto row x_rows_total - 1), which must be
# FINITE.  A block owns [128 co][128 ci] x KWB taps (2, or 1 for Kw = 1) x the steps [split sps, (split + 1) sps) of the
# N tsteps steps, sps = ceil(N tsteps / splits); with splits > 1 the blocks add atomically onto a zero-filled dw.

WGRAD8_DEFECTS = ('tap_frame_shifted', 'lane_group_dropped_h0', 'lane_group_dropped_h1', 'lane_group_dropped_h2', 'lane_group_dropped_h3',
                  'chunk_halves_swapped', 'odd_last_tap_second_window', 'split_last_step_dropped', 'accumulate_ignored_under_atomics',
                  'descale_dev_ignored', 'clamped_column_leaks')


@dataclasses.dataclass(frozen=True)
class Wgrad8Case:
    name: str
    N: int
    T: int                 # Tout
    Cin: int
    Cout: int
    Kw: int
    dil: int = 1
    gap: int = 0           # x rows between utterances beyond what one needs
    x_tail: int = 0        # live x rows behind the last utterance's stride (0: the buffer ends at the last row a live product reads)
    seed: int = 1

    @property
    def hb(self):
        return (self.Kw - 1) * self.dil

    @property
    def need(self):                     # x rows an utterance's live products read
        return self.T + self.hb

    @property
    def per(self):                      # x rows per utterance
        return self.need + self.gap

    @property
    def x_rows_total(self):
        return (self.N - 1) * self.per + self.need + self.x_tail

    @property
    def tsteps(self):
        return -(-self.T // BT)

    @property
    def steps(self):
        return self.N * self.tsteps

    @property
    def dy_per(self):                   # dy rows per utterance: the engine's shared-halo layout, halo = max(hb, dead frames)
        return self.T + max(self.hb, self.tsteps * BT - self.T)

    @property
    def dy_rows(self):
        return self.hb + self.N * self.dy_per

    @property
    def kwb(self):
        return 2 if self.Kw > 1 else 1

    @property
    def xrows(self):                    # rows of the staged x window
        return (BT + (self.kwb - 1) * self.dil + 7) & ~7

    @property
    def K(self):
        return self.N * self.T

    @property
    def key(self):                      # the tune cache's key
        return (self.N, self.Cin, self.Cout, self.T, self.Kw)

    @property
    def max_splits(self):
        return min(16, self.steps)


W1 = Wgrad8Case('W1_two_steps_odd_kw', 3, 130, 64, 192, 3, 1, gap=5, x_tail=320, seed=101)
W2 = Wgrad8Case('W2_one_frame_one_tap', 1, 1, 128, 64, 1, 1, seed=102)
W3 = Wgrad8Case('W3_no_dead_frames_d32', 2, 128, 192, 128, 2, 32, seed=103)
W4 = Wgrad8Case('W4_15_steps_d3', 5, 257, 64, 64, 4, 3, seed=104)
W5 = Wgrad8Case('W5_window_145_rows', 2, 75, 128, 128, 3, 17, seed=105)
W6 = Wgrad8Case('W6_shared_halo_x_clamped', 3, 130, 64, 192, 3, 1, seed=106)
WGRAD8_CASES = [W1, W2, W3, W4, W5, W6]


def wgrad8_plans(c):
    """(splits, order): every split count a loaded tune file can name, both block orders"""
    return [(s, o) for s in range(1, c.max_splits + 1) for o in (0, 1)]


def tune_line(c, splits, order):
    return 'wgradf8 %d %d %d %d %d %d %d\n' % (c.key + (splits, order))


TUNE_HEADER = 'w2l-tune v2 gfx950\n'


def make_wgrad8_case(c, family):
    """operands of a case as the device receives them:
    x  uint8 [x_rows_total][Cin]: codes of the family in EVERY row (the rows beneath dead frames, the gap rows and the tail are live
       data: the kernel multiplies them by the zero dy rows);
    dy uint8 [dy_rows][Cout]: utterance n at row hb + n dy_per: codes in its T rows, ZERO codes in rows [T, 128 tsteps), NAN8 in
       every row no step covers (the hb rows before utterance 0, rows from 128 tsteps to the next utterance);
    dw0 fp32 [Kw][Cout][Cin]: the accumulate operand (exact family: multiples of 2^-4 below 2^10)."""
    rng = np.random.default_rng(c.seed + (0 if family == 'exact' else 1000))
    x = codes(family, rng, (c.x_rows_total, c.Cin))
    dy = np.full((c.dy_rows, c.Cout), NAN8, dtype=np.uint8)
    for n in range(c.N):
        r = c.hb + n * c.dy_per
        dy[r: r + c.T] = codes(family, rng, (c.T, c.Cout))
        dy[r + c.T: r + c.tsteps * BT] = 0
    if family == 'exact':
        dw0 = (rng.integers(-2 ** 14 + 1, 2 ** 14, size=(c.Kw, c.Cout, c.Cin)) * 2.0 ** -4).astype(np.float32)
    else:
        dw0 = (rng.standard_normal((c.Kw, c.Cout, c.Cin)) * np.sqrt(c.K) * 1e4 * FACTORS['full'][0] * FACTORS['full'][1]).astype(np.float32)
    return dict(x=x, dy=dy, dw0=dw0, family=family)


def exact_units(K, unit=EXACT_UNIT, added=2.0 ** 10):
    """the largest magnitude an exact-family result or partial sum can reach, in units of the result's smallest unit: 16 K from the
    dot product, `added` (the bound of |dw0| / |bias| / |residual|) on top"""
    return 16 * K + added / unit


def _dy_frames(c, D):
    """float64 [N][128 tsteps][Cout]: the dy rows the kernel walks"""
    dy = E4M3[D['dy'][c.hb:]].reshape(c.N, c.dy_per, c.Cout)[:, :c.tsteps * BT]
    assert np.isfinite(dy).all() and not dy[:, c.T:].any()
    return dy


def _x_rows(c, D, rows):
    """float64 x rows (clamped onto the buffer, as the staging clamps them)"""
    return E4M3[D['x']][np.clip(rows, 0, c.x_rows_total - 1)]


def wgrad8_sums(c, D, defect=None, splits=1):
    """(S, A) float64 [Kw][Cout][Cin]: the sum of products and the sum of their magnitudes, before any factor.  defect: one of the
    index defects of WGRAD8_DEFECTS (the others act in wgrad8_ref):
        tap_frame_shifted           the last tap meets frame t - 1 of x (t + 1 for Kw = 1)
        lane_group_dropped_h<h>     frames 32 h .. 32 h + 7 of step 0 (lane group g = 0 of read h) contribute nothing
        chunk_halves_swapped        the last 16-byte chunk of ci: channel c takes the x bytes of channel c ^ 8
        odd_last_tap_second_window  the one-tap last group of an odd Kw reads its group's second-tap window: x row t + Kw dil
        split_last_step_dropped     splits whose steps_per_split rounds up: split 0 loses its last step
        clamped_column_leaks        a half-filled co tile: the last 16 live co take dy channels Cout - 32 .. Cout - 17"""
    dy = _dy_frames(c, D)
    F = c.tsteps * BT
    live = np.ones((c.N, F), dtype=bool)            # dead frames multiply zero dy rows: leaving them in changes nothing
    if defect is not None and defect.startswith('lane_group_dropped_h'):
        h = int(defect[-1])
        live[0, 32 * h: 32 * h + 8] = False
    if defect == 'split_last_step_dropped':
        sps = -(-c.steps // splits)
        if sps * splits > c.steps and sps > 1:
            n, ts = divmod(sps - 1, c.tsteps)
            live[n, ts * BT: (ts + 1) * BT] = False
    dyl = dy * live[:, :, None]
    if defect == 'clamped_column_leaks' and c.Cout % TILE == 64:
        dyl = dyl.copy()
        dyl[:, :, -16:] = dyl[:, :, -32:-16]
    S = np.zeros((c.Kw, c.Cout, c.Cin))
    A = np.zeros((c.Kw, c.Cout, c.Cin))
    t = np.arange(F)
    for k in range(c.Kw):
        off = k * c.dil
        if defect == 'tap_frame_shifted' and k == c.Kw - 1:
            off += -1 if c.Kw > 1 else 1
        if defect == 'odd_last_tap_second_window' and c.Kw > 1 and c.Kw % 2 == 1 and k == c.Kw - 1:
            off += c.dil
        for n in range(c.N):
            xw = _x_rows(c, D, n * c.per + t + off)
            if defect == 'chunk_halves_swapped':
                xw = xw.copy()
                xw[:, -16:] = xw[:, c.Cin - 16 + (np.arange(16) ^ 8)]
            S[k] += dyl[n].T @ xw
            A[k] += np.abs(dyl[n]).T @ np.abs(xw)
    return S, A


def wgrad_c(splits, accumulate, descale_dev):
    """roundings outside the dot product, from conv_wgrad_fp8.hip's epilogue: scale = descale * *descale_dev (one, with a device
    factor); acc * scale (one per block); the stores: splits - 1 atomic adds that can round (the first lands on an exact zero), one
    more where dw0 was there first"""
    return int(descale_dev) + 1 + (splits - 1) + int(accumulate)


def wgrad8_finish(c, D, S, A, splits=1, accumulate=False, descale_dev=True, defect=None, margin=None):
    """(v, bound) from the raw sums: the factors, the accumulate operand, and the bound (M K + c) u A"""
    ds, dd = FACTORS[D['family']]
    scale = ds * (dd if descale_dev and defect != 'descale_dev_ignored' else 1.0)
    v, A = S * scale, A * abs(scale)
    if accumulate and not (defect == 'accumulate_ignored_under_atomics' and splits > 1):
        v, A = v + D['dw0'].astype(np.float64), A + np.abs(D['dw0'].astype(np.float64))
    m = F8_DOT_MARGIN if margin is None else margin
    return v, (m * c.K + wgrad_c(splits, accumulate, descale_dev)) * U * A


def wgrad8_ref(c, D, splits=1, accumulate=False, descale_dev=True, defect=None, margin=None):
    S, A = wgrad8_sums(c, D, defect=defect, splits=splits)
    return wgrad8_finish(c, D, S, A, splits, accumulate, descale_dev, defect, margin)


def wgrad8_defect_applies(c, defect, splits=1, accumulate=False, descale_dev=True):
    """can this defect change what this launch of this case produces?"""
    if defect == 'tap_frame_shifted':
        return c.x_rows_total > 1                    # (one row in all: the neighbour frame is clamped onto it)
    if defect.startswith('lane_group_dropped_h'):
        return 32 * int(defect[-1]) < c.T
    if defect == 'odd_last_tap_second_window':
        return c.Kw > 1 and c.Kw % 2 == 1
    if defect == 'split_last_step_dropped':
        sps = -(-c.steps // splits)
        return sps * splits > c.steps and sps > 1
    if defect == 'accumulate_ignored_under_atomics':
        return accumulate and splits > 1
    if defect == 'descale_dev_ignored':
        return descale_dev
    if defect == 'clamped_column_leaks':
        return c.Cout % TILE == 64
    return True


WGRAD8_PATHS = ('two steps per utterance', 'dead frames', 'no dead frames', 'one live frame in the last step', 'one step in all',
                'odd Kw: one-tap last group', 'KWB = 1 build', 'half-filled co tile', 'ci tile of 64', 'window of 160 rows: five x groups',
                'partial last x group', 'tap x dil odd', 'tap x dil even', 'ragged steps_per_split', 'empty trailing split',
                'split crosses utterances', 'clamped staging', 'whole window on the last step')


def wgrad8_paths(c):
    """the paths of conv_wgrad_fp8.hip a case reaches over wgrad8_plans(c), from the launcher's own arithmetic restated"""
    p = set()
    dead = c.tsteps * BT - c.T
    if c.tsteps == 2:
        p.add('two steps per utterance')
    p.add('dead frames' if dead else 'no dead frames')
    if c.T - (c.tsteps - 1) * BT == 1:
        p.add('one live frame in the last step')
    if c.steps == 1:
        p.add('one step in all')
    if c.Kw > 1 and c.Kw % 2:
        p.add('odd Kw: one-tap last group')
    if c.kwb == 1:
        p.add('KWB = 1 build')
    if c.Cout % TILE == 64:
        p.add('half-filled co tile')
    if c.Cin % TILE == 64:
        p.add('ci tile of 64')
    groups = c.xrows // 8                                # eight-row groups of the window, dealt wave + 4 i
    if groups == 20:
        p.add('window of 160 rows: five x groups')
    elif groups % 4:
        p.add('partial last x group')
    if c.kwb == 2:
        p.add('tap x dil odd' if c.dil % 2 else 'tap x dil even')
    for s in range(1, c.max_splits + 1):
        sps = -(-c.steps // s)
        if sps * s > c.steps and sps > 1:
            p.add('ragged steps_per_split')
        if (s - 1) * sps >= c.steps:
            p.add('empty trailing split')
        if any(b // c.tsteps != (min(b + sps, c.steps) - 1) // c.tsteps for b in range(0, c.steps, sps)):
            p.add('split crosses utterances')
    # the staging of the last utterance's last step, first tap group: the whole window exists, or rows are clamped
    xrow0 = (c.N - 1) * c.per + (c.tsteps - 1) * BT
    p.add('whole window on the last step' if xrow0 + (c.Kw - 1) // c.kwb * c.kwb * c.dil + c.xrows - 1 <= c.x_rows_total - 1 else 'clamped staging')
    return p


# what each case is there for (the CPU test asserts wgrad8_paths(case) >= these, and that the union is WGRAD8_PATHS)
WGRAD8_CASE_PATHS = {
    W1.name: {'two steps per utterance', 'dead frames', 'odd Kw: one-tap last group', 'half-filled co tile', 'ci tile of 64',
              'whole window on the last step', 'tap x dil odd', 'empty trailing split'},
    W2.name: {'KWB = 1 build', 'one live frame in the last step', 'one step in all', 'clamped staging'},
    W3.name: {'no dead frames', 'window of 160 rows: five x groups', 'tap x dil even'},
    W4.name: {'ragged steps_per_split', 'empty trailing split', 'split crosses utterances', 'tap x dil odd',
              'one live frame in the last step', 'ci tile of 64'},
    W5.name: {'partial last x group', 'tap x dil odd', 'dead frames', 'odd Kw: one-tap last group'},
    W6.name: {'clamped staging', 'two steps per utterance', 'half-filled co tile'},
}


# ================================================================================================================================
# B. the forward / data-gradient convolution (conv_igemm_kernel<..., F8>, EPI = 0)
#
#   y[n][t][co] = descale (*descale_dev) sum_{k,ci} wq[k][co][ci] xq[n][t + k dil][ci]  (+ bias[co]);   statistics rows: one per
#   128-column tile of an utterance, row n tiles128 + j = (sum y, sum y^2) over the live columns of that tile.

# the block shapes of the e4m3 kernel: indices into conv_refs.SHAPES (conv_igemm.hip: kF8Cfgs)
F8_CFGS = (2, 5, 12, 14, 16, 1, 3, 8, 9, 11, 13, 18, 19, 21, 24)
NF8 = len(F8_CFGS)
LDS_BYTES = 160 * 1024
F8_PLAIN, F8_STATS, F8_FUSED = 0, 1, 3           # the statistics flags w2l_conv_plan_fp8 takes

CONV8_DEFECTS = ('next_utterance_row', 'one_product_dropped', 'last_row_dropped', 'dead_rows_counted', 'bias_not_in_stats',
                 'descale_dev_ignored')

F1 = C.ConvCase('F1_row_gap', 3, 128, 192, 5, 1, 2, 141, gap=4, seed=111)
F2 = C.ConvCase('F2_1x1', 5, 256, 64, 1, 1, 1, 97, seed=112)
F3 = C.ConvCase('F3_19_columns', 12, 128, 128, 7, 1, 4, 19, seed=113)
F4 = C.ConvCase('F4_nine_k_steps', 2, 384, 320, 3, 1, 1, 300, seed=114)
CONV8_CASES = [F1, F2, F3, F4]
SENT8 = 0x7E                                       # +448: what fills the x rows no live output reads (gap rows, the rows after the last)


def f8_shape(k):
    return C.SHAPES[F8_CFGS[k]]


def f8_cols(k):
    _, nw, _, ns = f8_shape(k)
    return 16 * nw * ns


def f8_fused_built(k):
    """the fused form is not built for the four shapes whose epilogue spills (conv_igemm.hip: f8_fused_built)"""
    _, nw, ms, ns = f8_shape(k)
    return not ((ms == 6 and ns == 4) or ms == 8 or (nw == 3 and ns == 6))


def f8_cannot_run(c, k, flag):
    """the documented reason for which forced block shape k cannot run this problem under this statistics flag, or None"""
    mw, nw, ms, ns = f8_shape(k)
    if flag == F8_FUSED and not f8_fused_built(k):
        return 'not built for the fused epilogue'
    if flag == F8_STATS and f8_cols(k) not in (128, 256):
        return 'tile rows need 128 / 256 columns'
    xrows = ((f8_cols(k) - 1) + (c.Kw - 1) * c.dil + 1 + 7) & ~7
    if 2 * 16 * mw * ms * 128 + 2 * xrows * 128 > LDS_BYTES:
        return 'LDS'
    return None


# which (case, flag, block shape) runs: 'r' runs, 'f' not built for the fused epilogue, 't' tile rows need 128 / 256 columns,
# 'L' LDS.  tests/test_cpu_fp8_refs.py pins this table to f8_cannot_run and to w2l_conv_plan_fp8
F8_CODE = {None: 'r', 'not built for the fused epilogue': 'f', 'tile rows need 128 / 256 columns': 't', 'LDS': 'L'}
F8_FEASIBLE = {
    'F1_row_gap': {0: 'rrrrrrrrrrrrrrr', 1: 'rrrrrrrttrrtttt', 3: 'rrrffrrrrrrffrr'},
    'F2_1x1': {0: 'rrrrrrrrrrrrrrr', 1: 'rrrrrrrttrrtttt', 3: 'rrrffrrrrrrffrr'},
    'F3_19_columns': {0: 'rrrrrrrrrrrrrrr', 1: 'rrrrrrrttrrtttt', 3: 'rrrffrrrrrrffrr'},
    'F4_nine_k_steps': {0: 'rrrrrrrrrrrrrrr', 1: 'rrrrrrrttrrtttt', 3: 'rrrffrrrrrrffrr'},
}


def make_conv8_case(c, family):
    """operands of a case as the device receives them: x uint8 [x_rows_total][Cin] (codes of the family in the rows a live output
    reads, SENT8 = +448 in every other row); w uint8 [Cout][Cin][Kw] (w_device8: the kernel's [Kw][Cout][Cin]); bias fp32 (exact
    family: multiples of 2^-4 up to 64)"""
    rng = np.random.default_rng(c.seed + (0 if family == 'exact' else 1000))
    x = np.full((c.x_rows_total, c.Cin), SENT8, dtype=np.uint8)
    for n in range(c.N):
        x[n * c.per: n * c.per + c.need] = codes(family, rng, (c.need, c.Cin))
    w = codes(family, rng, (c.Cout, c.Cin, c.Kw))
    if family == 'exact':
        bias = (rng.integers(-2 ** 10, 2 ** 10 + 1, size=c.Cout) * 2.0 ** -4).astype(np.float32)
    else:
        bias = (rng.standard_normal(c.Cout) * np.sqrt(c.K) * 1e4 * FACTORS['full'][0] * FACTORS['full'][1]).astype(np.float32)
    return dict(x=x, w=w, bias=bias, family=family)


def w_device8(D, flipped=False):
    """[Kw][Cout][Cin] bytes; flipped: the taps in reverse order (the data gradient's operand)"""
    w = D['w'].transpose(2, 0, 1)
    return np.array(w[::-1] if flipped else w, order='C')


def bound_of(tr, r_out=0.0):
    """(d + 2) u a (+ r_out |v|) of a tracked value: Tr.bound() without its sanity limit on d, which F8_DOT_MARGIN x Kw Cin exceeds"""
    return (tr.d + 2) * U * tr.a + r_out * np.abs(tr.v)


def conv_c(bias, descale_dev):
    """roundings outside the dot product, from the epilogue: descale * *descale_dev (one, with a device factor), acc * descale (one),
    + bias (one, with a bias)"""
    return int(descale_dev) + 1 + int(bias)


def _finish8(raw, family, K, bias, descale_dev, ignore_dd=False, margin=None):
    """Tr of descale (*descale_dev) raw (+ bias) whose bound() is (M K + c) u A"""
    ds, dd = FACTORS[family]
    scale = ds * (dd if descale_dev and not ignore_dd else 1.0)
    v, a = raw.v * scale, raw.a * abs(scale)
    if bias is not None:
        b = np.asarray(bias, dtype=np.float64)
        v, a = v + b, a + np.abs(b)
    m = F8_DOT_MARGIN if margin is None else margin
    out = Tr(v, a, int(np.ceil(m * K)) + conv_c(bias is not None, descale_dev) - 2)
    out.c8 = conv_c(bias is not None, descale_dev)          # c of this launch form, for the GPU test's margin-1 figure (K + c) u A
    return out


def conv8_ref(c, D, flipped=False, bias=True, descale_dev=True, defect=None, rows=None, margin=None):
    """Tr [N][Tout][Cout] of one launch form.  defect: next_utterance_row / one_product_dropped (conv_refs.conv_fwd_ref) or
    descale_dev_ignored; rows: as conv_fwd_ref (the dead columns of the last tile)"""
    xf = E4M3[D['x']]
    wf = E4M3[D['w']]
    if flipped:
        wf = wf[:, :, ::-1]
    raw = C.conv_fwd_ref(xf[:c.N * c.per].reshape(c.N, c.per, c.Cin), wf, None, c.Tout, 1, c.dil,
                         defect=defect if defect in C.ELEMENT_DEFECTS else None, rows=rows,
                         x_tail=xf[c.N * c.per:] if rows is not None else None)
    return _finish8(raw, D['family'], c.K, D['bias'] if bias else None, descale_dev, ignore_dd=defect == 'descale_dev_ignored',
                    margin=margin)


def conv8_stats(c, D, v, k, defect=None, descale_dev=True):
    """(s1, s2) Tr [Cout] of the statistics launch (bias, the given device factor) under block shape k"""
    depth = C.stats_sum_depth(F8_CFGS[k], c.N, c.Tout, 0)
    dead = conv8_ref(c, D, descale_dev=descale_dev, rows=C.dead_rows(c)) if defect == 'dead_rows_counted' else None
    return C.conv_stats_ref(v, depth, defect=defect, dead=dead, bias=D['bias'])


def tile_row_sums(c, y):
    """float64 [N tiles128][Cout]: the sums over the live columns of every 128-column tile, row n tiles128 + j"""
    t128 = -(-c.Tout // 128)
    return np.stack([y[n, j * 128: (j + 1) * 128].sum(0) for n in range(c.N) for j in range(t128)])


def conv8_defect_applies(c, defect, descale_dev=True):
    if defect == 'descale_dev_ignored':
        return descale_dev
    return C.conv_defect_applies(c, defect)


# ================================================================================================================================
# C. the fused inference epilogue on e4m3 operands (conv_igemm_kernel<..., F8, EPI = 2>), on the exact family: the accumulator
# v = acc descale + bias is then known exactly (descale a power of two, bias a multiple of 2^-4), and the whole error is the
# epilogue's: v scale + shift (two roundings), + res (one), the activation, the mask; stored as bf16 and / or as e4m3 of a q_scale.

FUSED8_DESCALE = FACTORS['exact'][0]               # the fused launch takes no device factor


def fused8_variants(c):
    """the cases of tests/test_gpu_infer_fp8._cases on this geometry, as conv_refs.Fused: (variant, bias, q_scale)"""
    pad = (c.Kw - 1) * c.dil
    out = [(C.Fused('w2l', pad // 2, pad - pad // 2, 1, act=1), True, 16.0),
           (C.Fused('jasper', max(pad // 2, 1), max(pad // 2, 1), 0, act=2, lens='ragged'), False, 8.0),
           (C.Fused('jasper_res', 28, 28, 0, act=2, lens='ragged', res=1), False, 8.0)]
    if c.Kw == 1:
        out.append((C.Fused('dense_1x1', act=0, tail=0), False, 8.0))
    return out


FUSED8_CASES = [F1, F2, F3]


def make_fused8_params(c, f):
    """scale ~ 1 / (the accumulator's spread), so that the unit's output is O(1); shift N(0,1) with every seventh channel near the
    clamp's upper edge; res bf16; ragged lens"""
    rng = np.random.default_rng(c.seed * 7 + sum(map(ord, f.name)))
    spread = np.sqrt(c.K * (20.0 / 3.0) ** 2) * FUSED8_DESCALE           # a product of two uniform [-4, 4] integers has variance (20/3)^2
    shift = rng.standard_normal(c.Cout)
    shift[::7] += 19.0
    return dict(scale=((0.5 + rng.random(c.Cout)) / spread).astype(np.float32), shift=shift.astype(np.float32),
                res=C.bf16(rng.standard_normal((c.N, c.Tout, c.Cout)) * 2) if f.res else None,
                lens=C.conv_lens(f.lens, c.N, c.Tout))


def fused8_acc(c, D, bias):
    """the exact v = acc descale (+ bias) [N][Tout][Cout] of the exact family"""
    assert D['family'] == 'exact'
    xf, wf = E4M3[D['x']], E4M3[D['w']]
    raw = C.conv_fwd_ref(xf[:c.N * c.per].reshape(c.N, c.per, c.Cin), wf, None, c.Tout, 1, c.dil)
    v = raw.v * FUSED8_DESCALE + (D['bias'].astype(np.float64) if bias else 0.0)
    assert np.array_equal(v, v.astype(np.float32))
    return v


def fused8_ref(c, f, P, v, q_scale, defect=None):
    """dict: a (Tr [N][out_rows][Cout], NaN in the rows never written), aq (Tr of a q_scale: round with e4m3_bound), src, rows"""
    rows = f.pad_l + c.Tout + f.pad_r
    out = C.infer_ref(v, P['scale'], P['shift'], P['res'], None, f.act, P['lens'], rows + f.tail, f.pad_l, f.pad_r, f.pad_mode,
                      defect=defect)
    a = out['a']
    out['aq'] = Tr(a.v, a.a, a.d) * Tr(f32(q_scale))
    out['rows'] = rows
    return out


def e4m3_certain(aq, bound):
    """(codes, sure): e4m3_rne_sat of the reference, and where the code is certain -- the reference farther from a rounding boundary
    than the fp32 error it may carry, so that both ends of [ref - bound, ref + bound] round to the same code"""
    lo, hi, mid = e4m3_rne_sat(aq - bound), e4m3_rne_sat(aq + bound), e4m3_rne_sat(aq)
    zero = lambda q: (q & 0x7F) == 0
    sure = ((lo == mid) & (hi == mid)) | (zero(lo) & zero(hi))
    return mid, sure
