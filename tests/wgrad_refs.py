"""Float64 reference of the dense Conv1d weight gradient (csrc/conv_wgrad_kernel.h, conv_wgrad.hip, conv_wgrad3_dev.hip) -- plain
NumPy, nothing of the engine's Python -- with the cases, operands, planted defects and forced plans that
tests/test_cpu_wgrad_refs.py (no GPU) and tests/test_gpu_wgrad_direct.py share.

    dw[k][co][ci] = sum_{n, t < Tout} dy[n][t][co] x[n][t*stride + k*dil][ci]   (+ dw0[k][co][ci] with accumulate = 1)

The bound.  Both operands are bf16 values, so every product is exact in fp32 (8 + 8 significand bits).  Any summation order of
the d = N Tout products -- MFMA accumulation chains, K steps, splits, slabs summed in range order, atomics in arrival order --
takes a term through at most d - 1 additions that round; adding an exact zero (the dead rows of a last step, an idle tap) does
not round.  So |device - v| <= (d + 2) u A per element (kernel_refs.Tr.bound), A the same sum on absolute values; the
accumulate operand is one more term: v += dw0, A += |dw0|, d += 1.  WGRAD_DOT_MARGIN multiplies the bound: the one number that
is measured (tests/test_gpu_wgrad_direct.py::test_plain_plan_obeys_its_bound), not derived.

The planted defects (WGRAD_DEFECTS) are mistakes that a whole-tensor relative error of 2e-3 cannot see; the CPU test proves each
one lies outside the bound on every case where wgrad_defect_applies() holds."""
import dataclasses

import numpy as np

from bn_refs import SENTINEL
from kernel_refs import Tr, U, bf16_rne, bf16_to_f32  # noqa: F401  (re-exported)

# the factor on the bound: 1 = the fp32 accumulation of the matrix unit obeys (N Tout + 2) u A against float64.  Measured on
# an MI355X by test_plain_plan_obeys_its_bound: the worst error / bound of the unsplit two-tap plan (order 1, count 1) over the
# six cases is 0.0100 (case C; 0.0106 over every family), so the bound needs no widening.
WGRAD_DOT_MARGIN = 1.0

BT, TILE = 64, 128            # rows of a K step, channels of a tile (conv_wgrad_kernel.h: BT, BM = BNC)

WGRAD_DEFECTS = ('one_product_dropped', 'last_row_dropped', 'next_utterance_row', 'tail_row_clamped_early', 'edge_channels_shifted',
                 'last_tap_from_idle_group', 'accumulate_dropped_in_edge_tile')


def bf16(x):
    """the nearest bf16 value, as float32"""
    return bf16_to_f32(bf16_rne(np.asarray(x, dtype=np.float32)))


def roundup64(t):
    return -(-t // BT) * BT


# ---- the reference -----------------------------------------------------------------------------------------------------------------

def wgrad_ref(dy, x, Tout, stride, dil, Kw, dw0=None, defect=None):
    """Tr [Kw][Cout][Cin].  dy [N][rows >= Tout][Cout], x [N][per][Cin]: the bf16 values exactly as uploaded (per >= the rows an
    utterance needs); dw0 [Kw][Cout][Cin]: the fp32 operand of accumulate = 1.  defect: one of WGRAD_DEFECTS (module docstring
    of tests/test_gpu_wgrad_direct.py says what each one stands for)."""
    dy = np.asarray(dy, dtype=np.float64)[:, :Tout]
    x = np.asarray(x, dtype=np.float64)
    N, per, Cin = x.shape
    Cout = dy.shape[2]
    need = (Tout - 1) * stride + (Kw - 1) * dil + 1
    assert per >= need and dy.shape[:2] == (N, Tout)
    if defect == 'next_utterance_row':             # utterance n starts at row n * need of the buffer, not at n * per
        flat = x.reshape(N * per, Cin)
        x = np.stack([flat[n * need: n * need + need] for n in range(N)])
    elif defect == 'tail_row_clamped_early':       # x_max_row one too small: the last live row of the buffer is the one before it
        x = x.copy()
        x[N - 1, need - 1] = x[N - 1, need - 2]

    def window(k):                                 # [N][Tout][Cin]: the rows tap k meets
        return x[:, k * dil: k * dil + (Tout - 1) * stride + 1: stride]

    v = np.zeros((Kw, Cout, Cin))
    A = np.zeros((Kw, Cout, Cin))
    ady = np.abs(dy)
    for k in range(Kw):
        win = window(k)
        v[k] = np.einsum('ntc,nti->ci', dy, win)
        A[k] = np.einsum('ntc,nti->ci', ady, np.abs(win))
    d = N * Tout
    if defect == 'one_product_dropped':            # the largest product of the last element
        term = dy[:, :, -1] * window(Kw - 1)[:, :, -1]
        term = term.reshape(-1)[np.abs(term).argmax()]
        v[-1, -1, -1] -= term
        A[-1, -1, -1] -= abs(term)
    elif defect == 'last_row_dropped':             # row Tout - 1 of the last utterance, in the last 128-channel ci tile only
        ci0 = (-(-Cin // TILE) - 1) * TILE
        for k in range(Kw):
            row = np.outer(dy[N - 1, Tout - 1], window(k)[N - 1, Tout - 1, ci0:])
            v[k, :, ci0:] -= row
            A[k, :, ci0:] -= np.abs(row)
    elif defect == 'last_tap_from_idle_group' and Kw > 1:
        v[-1], A[-1] = v[-2], A[-2]
    elif defect == 'edge_channels_shifted':        # the staging clamp (Cin - 8 / Cout - 8) leaking into stored elements
        if Cin % TILE == 64:
            v[:, :, -8:], A[:, :, -8:] = v[:, :, -16:-8], A[:, :, -16:-8]
        if Cout % TILE == 64:
            v[:, -8:, :], A[:, -8:, :] = v[:, -16:-8, :], A[:, -16:-8, :]
    if dw0 is not None:
        a0 = np.asarray(dw0, dtype=np.float64)
        a = a0
        if defect == 'accumulate_dropped_in_edge_tile':                 # dw0 is not added in the last co tile
            a = a0.copy()
            a[:, (-(-Cout // TILE) - 1) * TILE:] = 0.0
        v, A, d = v + a, A + np.abs(a), d + 1
    return Tr(v, A, d)


# ---- the cases ---------------------------------------------------------------------------------------------------------------------

@dataclasses.dataclass(frozen=True)
class WgradCase:
    name: str
    N: int
    Cin: int
    Cout: int
    Kw: int
    stride: int
    dil: int
    Tout: int
    gap: int = 0          # x rows between utterances beyond what one needs
    seed: int = 1

    @property
    def need(self):
        return (self.Tout - 1) * self.stride + (self.Kw - 1) * self.dil + 1

    @property
    def per(self):                      # x rows per utterance
        return self.need + self.gap

    @property
    def x_rows_total(self):             # the buffer ends with the last utterance's stride: exactly at its last needed row if gap = 0
        return self.N * self.per

    @property
    def hb(self):                       # dy rows before utterance 0
        return (self.Kw - 1) * self.dil

    @property
    def dy_per(self):                   # dy rows per utterance (the shared-halo layout: halo = max(hb, the dead rows of the last step))
        return self.Tout + max(self.hb, roundup64(self.Tout) - self.Tout)

    @property
    def dy_rows(self):
        return self.hb + self.N * self.dy_per

    @property
    def steps(self):                    # K steps in all: S
        return self.N * (roundup64(self.Tout) // BT)

    @property
    def K(self):
        return self.N * self.Tout

    @property
    def shape(self):
        return (self.N, self.Cin, self.Cout, self.Tout, self.Kw, self.stride, self.dil)


# the smallest shapes that still reach each edge; K = N Tout <= 520 keeps one dropped product far outside the bound (it fades as
# 1 / (K^2 u))
WGRAD_A = WgradCase('A_one_live_row', 3, 192, 192, 7, 1, 1, 65, gap=4, seed=71)
WGRAD_B = WgradCase('B_63_live_rows_dil4', 2, 64, 128, 5, 1, 4, 127, seed=72)
WGRAD_C = WgradCase('C_stride2', 2, 64, 192, 3, 2, 1, 70, seed=73)
WGRAD_D = WgradCase('D_one_tap', 5, 192, 64, 1, 1, 1, 64, seed=74)
WGRAD_E = WgradCase('E_dil5_one_utterance', 1, 128, 128, 6, 1, 5, 200, seed=75)
WGRAD_F = WgradCase('F_12_steps', 4, 128, 128, 8, 1, 2, 130, seed=76)
WGRAD_CASES = [WGRAD_A, WGRAD_B, WGRAD_C, WGRAD_D, WGRAD_E, WGRAD_F]

# the layers of the group launch (Cin, Cout, Kw) at N = 3, Tout = 65, dilation 1 and 2
GROUP_LAYERS = [(192, 192, 7), (64, 128, 5), (192, 64, 1), (128, 128, 9)]
GROUP_N, GROUP_TOUT, GROUP_DILS = 3, 65, (1, 2)
FORMS = (0, 1, 4, 5, 8, 9, 16, 17, 20, 21)
GROUP_SELECTIONS = ([0], [3], [0, 1], [2, 1], [0, 1, 2, 3], [3, 2, 1, 0])


def group_case(i, dil):
    Cin, Cout, Kw = GROUP_LAYERS[i]
    return WgradCase(f'G{i}_d{dil}', GROUP_N, Cin, Cout, Kw, 1, dil, GROUP_TOUT, gap=(0, 3, 0, 1)[i], seed=80 + 4 * dil + i)


def make_wgrad_case(c):
    """operands of a case, every value a bf16 value held in float32 (dw0: fp32):
    x  [x_rows_total][Cin]: N(0,1) in the rows an utterance needs, SENTINEL in the gap rows (the GPU test puts NaN rows behind it);
    dy [dy_rows][Cout]: utterance n at row hb + n dy_per: N(0,1) in its Tout rows, ZERO in rows [Tout, roundup64(Tout)) (the
       documented contract), SENTINEL in every row no utterance's 64-row steps cover: the hb rows before utterance 0 and the rows
       from roundup64(Tout) to the next utterance;
    dw0 [Kw][Cout][Cin]: the accumulate operand, of the gradient's own magnitude."""
    rng = np.random.default_rng(c.seed)
    x = np.full((c.x_rows_total, c.Cin), SENTINEL, dtype=np.float32)
    for n in range(c.N):
        x[n * c.per: n * c.per + c.need] = bf16(rng.standard_normal((c.need, c.Cin)))
    dy = np.full((c.dy_rows, c.Cout), SENTINEL, dtype=np.float32)
    for n in range(c.N):
        r = c.hb + n * c.dy_per
        dy[r: r + c.Tout] = bf16(rng.standard_normal((c.Tout, c.Cout)))
        dy[r + c.Tout: r + roundup64(c.Tout)] = 0.0
    dw0 = (rng.standard_normal((c.Kw, c.Cout, c.Cin)) * np.sqrt(c.K)).astype(np.float32)
    return dict(x=bf16(x), dy=bf16(dy), dw0=dw0)


def x_view(c, D):
    return D['x'].reshape(c.N, c.per, c.Cin)


def dy_view(c, D):
    return D['dy'][c.hb:].reshape(c.N, c.dy_per, c.Cout)


def wgrad_ref_of(c, D, dw0=False, defect=None):
    return wgrad_ref(dy_view(c, D), x_view(c, D), c.Tout, c.stride, c.dil, c.Kw, dw0=D['dw0'] if dw0 else None, defect=defect)


def margin(tr):
    """the bound the tests apply: WGRAD_DOT_MARGIN (d + 2) u A"""
    return WGRAD_DOT_MARGIN * tr.bound()


def wgrad_defect_applies(case, defect, dw0=False):
    """can this defect change what a launch of this case produces?
    one_product_dropped, last_row_dropped, tail_row_clamped_early: always;
    next_utterance_row: utterances further apart than their rows (per > need), N > 1;
    edge_channels_shifted: a half-filled edge tile, Cin % 128 == 64 or Cout % 128 == 64;
    last_tap_from_idle_group: a tap count that leaves a partial tap group under some block form (2, 3, 4 or 6 taps per block);
    accumulate_dropped_in_edge_tile: launches with accumulate = 1."""
    c = case
    if defect == 'next_utterance_row':
        return c.per > c.need and c.N > 1
    if defect == 'edge_channels_shifted':
        return c.Cin % TILE == 64 or c.Cout % TILE == 64
    if defect == 'last_tap_from_idle_group':
        return c.Kw > 1 and any(c.Kw % b for b in (2, 3, 4, 6))
    if defect == 'accumulate_dropped_in_edge_tile':
        return dw0
    return True


# ---- the forced plans of the GPU sweep and the path each one takes -------------------------------------------------------------------

PLAN_FIELDS = ('splits', 'steps_per_split', 'tsteps', 'total_steps', 'order', 'streamk', 'tg2', 'm32', 'taps3', 'kwb', 'kwblk', 'kgroups',
               'tiles', 'G', 'dealt_b', 'slabs', 'atomic', 'needs_zero', 'xrows_lds', 'lds', 'grid_x', 'grid_y', 'threads', 'ok')
STREAMK, DEALT, ATOMIC_WS = 2, 32, 64           # plan order bits 1, 5, 6 (include/w2l_hip.h: w2l_wgrad_force_plan)


def tiles2(c):
    """tiles of the two-tap form: the most any form has"""
    return -(-c.Cout // TILE) * -(-c.Cin // TILE) * -(-c.Kw // (2 if c.Kw > 1 else 1))


def wgrad_plans(c):
    """the forced (workspace, count, order) of the GPU sweep over one case, in the order of WGRAD_PATHS[c.name]:
    classic   counts {1, 2, 3, S} x the ten block forms, with and without a workspace;
    stream-K  orders {2, 3, 6, 7} without a workspace (with one the classic plan runs), and 2 / 6 with bit 6 and a workspace (count 1:
              a stream-K plan does not use it, and a pinned count keeps a remembered plan out of the choice);
    dealt     32 | form at two range counts between the tile count and tiles x S, and without a workspace (the fallback split);
    atomics although a workspace is given: 64 | 1 at 2 and S splits."""
    S = c.steps
    plans = [(ws, n, o) for ws in (True, False) for n in sorted({1, 2, 3, S}) for o in FORMS]
    plans += [(False, 1, o) for o in (2, 3, 6, 7)] + [(True, 1, ATOMIC_WS | o) for o in (2, 6)]
    plans += [(True, g, DEALT | o) for g in (tiles2(c) + 1, 2 * tiles2(c) + 1) for o in FORMS]
    plans += [(False, g, DEALT | 1) for g in (tiles2(c) + 1, 2 * tiles2(c) + 1)]
    plans += [(True, n, ATOMIC_WS | 1) for n in (2, S)]
    return plans


REDUCTIONS = {'u': 'unsplit', 's': 'slabs', 'a': 'atomic', 'k': 'stream-K 4-wave', 'K': 'stream-K 8-wave', 'd': 'dealt', 'f': 'dealt fallback'}
BLOCK_FORMS = {'1': 'taps1', '2': 'taps2', '4': 'taps4', 'm': 'm32', '3': 'taps3', '6': 'taps6'}
ALL_PATHS = tuple(REDUCTIONS.values()) + tuple(BLOCK_FORMS.values()) + ('narrowed',)


def wgrad_path(r, order):
    """the path of one launch as three characters: its reduction, the block form that RUNS, and '!' where the forced form bits
    asked for another kernel than the one that runs (narrowed) or '.'.  r: dict of PLAN_FIELDS, what w2l_wgrad_launch_plan says."""
    if r['G']:
        red = 'd'
    elif order & DEALT and not order & STREAMK:
        red = 'f'
    elif r['streamk']:
        red = 'K' if r['threads'] == 512 else 'k'
    else:
        red = 's' if r['slabs'] else 'a' if r['atomic'] else 'u'
        assert (red == 'u') == (r['splits'] == 1)
    form = ('6' if r['tg2'] else '3') if r['taps3'] else 'm' if r['m32'] else '4' if r['tg2'] else str(r['kwblk'])
    asked = (bool(order & STREAMK), bool(order & 4), bool(order & 8), bool(order & 16))
    runs = (bool(r['streamk']), bool(r['tg2']), bool(r['m32']), bool(r['taps3']))
    return red + form + ('.' if asked == runs else '!')


def path_names(code):
    """the names a path code counts under"""
    return [REDUCTIONS[code[0]], BLOCK_FORMS[code[1]]] + (['narrowed'] if code[2] == '!' else [])


def path_counts(codes):
    out = {}
    for code in codes:
        for name in path_names(code):
            out[name] = out.get(name, 0) + 1
    return out


# What w2l_wgrad_launch_plan answers for wgrad_plans(case), one code per plan, with the workspace
# max(w2l_wgrad_workspace_bytes, w2l_wgrad_dealt_workspace_bytes) of the layer.  tests/test_cpu_wgrad_refs.py asserts that the
# library still answers the same and that every path occurs; the GPU test's "really ran" counts are path_counts() of these.
WGRAD_PATHS = {
    'A_one_live_row': (
        'u2. u2. u4. u4. um. um. u3. u3. u6. u6. s2. s2. s4. s4. sm. sm. s3. s3. s6. s6. s2. s2. s4. s4. sm. sm. s3. s3. s6. s6. '
        's2. s2. s4. s4. sm. sm. s3. s3. s6. s6. u2. u2. u4. u4. um. um. u3. u3. u6. u6. a2. a2. a4. a4. am. am. a3. a3. a6. a6. '
        'a2. a2. a4. a4. am. am. a3. a3. a6. a6. a2. a2. a4. a4. am. am. a3. a3. a6. a6. k2. k2. K4. K4. k2. K4. d2. d2. d4. d4. '
        'dm. dm. d3. d3. d6. d6. d2. d2. d4. d4. dm. dm. d3. d3. d6. d6. f2. f2. a2. a2. '
    ),
    'B_63_live_rows_dil4': (
        'u2. u2. u4. u4. um. um. u3. u3. u6. u6. s2. s2. s4. s4. sm. sm. s3. s3. s6. s6. s2. s2. s4. s4. sm. sm. s3. s3. s6. s6. '
        's2. s2. s4. s4. sm. sm. s3. s3. s6. s6. u2. u2. u4. u4. um. um. u3. u3. u6. u6. a2. a2. a4. a4. am. am. a3. a3. a6. a6. '
        'a2. a2. a4. a4. am. am. a3. a3. a6. a6. a2. a2. a4. a4. am. am. a3. a3. a6. a6. k2. k2. K4. K4. k2. K4. d2. d2. d4. d4. '
        'dm. dm. d3. d3. d6. d6. d2. d2. d4. d4. dm. dm. d3. d3. f6. f6. f2. f2. a2. a2. '
    ),
    'C_stride2': (
        'u2. u2. u4. u4. u2! u2! u2! u2! u4! u4! s2. s2. s4. s4. s2! s2! s2! s2! s4! s4! s2. s2. s4. s4. s2! s2! s2! s2! s4! s4! '
        's2. s2. s4. s4. s2! s2! s2! s2! s4! s4! u2. u2. u4. u4. u2! u2! u2! u2! u4! u4! a2. a2. a4. a4. a2! a2! a2! a2! a4! a4! '
        'a2. a2. a4. a4. a2! a2! a2! a2! a4! a4! a2. a2. a4. a4. a2! a2! a2! a2! a4! a4! k2. k2. k2! k2! k2. k2! d2. d2. d4. d4. '
        'd2! d2! d2! d2! d4! d4! d2. d2. f4. f4. d2! d2! d2! d2! f4! f4! f2. f2. a2. a2. '
    ),
    'D_one_tap': (
        'u1. u1. u1! u1! um. um. u1! u1! u1! u1! s1. s1. s1! s1! sm. sm. s1! s1! s1! s1! s1. s1. s1! s1! sm. sm. s1! s1! s1! s1! '
        's1. s1. s1! s1! sm. sm. s1! s1! s1! s1! u1. u1. u1! u1! um. um. u1! u1! u1! u1! a1. a1. a1! a1! am. am. a1! a1! a1! a1! '
        'a1. a1. a1! a1! am. am. a1! a1! a1! a1! a1. a1. a1! a1! am. am. a1! a1! a1! a1! k1. k1. k1! k1! k1. k1! d1. d1. d1! d1! '
        'dm. dm. d1! d1! d1! d1! d1. d1. d1! d1! dm. dm. d1! d1! d1! d1! f1. f1. a1. a1. '
    ),
    'E_dil5_one_utterance': (
        'u2. u2. u4. u4. um. um. u2! u2! u4! u4! s2. s2. s4. s4. sm. sm. s2! s2! s4! s4! s2. s2. s4. s4. sm. sm. s2! s2! s4! s4! '
        's2. s2. s4. s4. sm. sm. s2! s2! s4! s4! u2. u2. u4. u4. um. um. u2! u2! u4! u4! a2. a2. a4. a4. am. am. a2! a2! a4! a4! '
        'a2. a2. a4. a4. am. am. a2! a2! a4! a4! a2. a2. a4. a4. am. am. a2! a2! a4! a4! k2. k2. K4. K4. k2. K4. d2. d2. d4. d4. '
        'dm. dm. d2! d2! d4! d4! d2. d2. d4. d4. dm. dm. d2! d2! d4! d4! f2. f2. a2. a2. '
    ),
    'F_12_steps': (
        'u2. u2. u4. u4. um. um. u3. u3. u6. u6. s2. s2. s4. s4. sm. sm. s3. s3. s6. s6. s2. s2. s4. s4. sm. sm. s3. s3. s6. s6. '
        's2. s2. s4. s4. sm. sm. s3. s3. s6. s6. u2. u2. u4. u4. um. um. u3. u3. u6. u6. a2. a2. a4. a4. am. am. a3. a3. a6. a6. '
        'a2. a2. a4. a4. am. am. a3. a3. a6. a6. a2. a2. a4. a4. am. am. a3. a3. a6. a6. k2. k2. K4. K4. k2. K4. d2. d2. d4. d4. '
        'dm. dm. d3. d3. d6. d6. d2. d2. d4. d4. dm. dm. d3. d3. d6. d6. f2. f2. a2. a2. '
    ),
}
WGRAD_PATHS = {k: v.split() for k, v in WGRAD_PATHS.items()}
