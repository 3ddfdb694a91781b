"""Float64 references of the implicit GEMM forward (csrc/conv_igemm.hip, EPI = 0: bias, fp32 / bf16 store, accumulate, the
BatchNorm partial sums) and of the fused inference epilogue (EPI = 2, w2l_conv1d_igemm_bnact) -- plain NumPy, nothing of the
engine's Python.  Values are tracked (kernel_refs.Tr: exact value, the expression on absolute values, roundings on the longest
path), so every bound a test applies is (depth + 2) u A of the operation actually performed, per element.

The sums.  conv_igemm.hip forms s1 = sum v, s2 = sum v*v over the live columns (t < Tout) of a block from the UNROUNDED fp32
value v (after bias and the accumulate operand).  The chain of additions one value goes through is short, whatever the row count:
    NS   a lane adds the NS column fragments it holds (one product more for s2),
    4    the sixteen column lanes of a fragment are combined by four exchanges,
    NW   (tile rows: NW / (BN / 128)) the column waves' sums are added from LDS,
    ceil(N * tiles_t / S)   slot rows only: the blocks whose column tile falls on one slot row add onto it (any order),
and the rows are summed on the host in float64.  stats_sum_depth() is that count; two bounds follow:
    full            the value v carries the dot product's depth (Kw Cin + 1 (+ 1)) and magnitude sum into the chain;
    epilogue alone  the fp32 store of the same configuration is taken as the EXACT input: depth = the chain alone (+ 1 for the
                    square), magnitude = sum |y| (sum y^2) -- nothing of the dot product, so one row in 16 000 is visible.

The planted defects (CONV_DEFECTS, ``defect=``) are the mistakes an epilogue or a K loop can make without the coarse tests
noticing; tests/test_cpu_conv_refs.py proves each one lies outside the bound wherever conv_defect_applies() says it can act."""
import dataclasses

import numpy as np

import bn_refs as B
from bn_refs import SENTINEL, bn_act_fwd_ref, lens_limits, pad_src_rows
from kernel_refs import R_BF16, R_SPLIT, Tr, U, bf16_rne, bf16_to_f32, dot_bound, split_bf16  # noqa: F401  (re-exported)

# the block shapes (mw, nw, ms, ns) of conv_igemm.hip in index order: BM = 16 mw ms channels x BN = 16 nw ns columns
SHAPES = [(2, 2, 2, 4), (2, 2, 3, 4), (2, 2, 4, 4), (2, 2, 5, 4), (4, 2, 3, 4), (4, 2, 4, 4), (2, 3, 2, 3), (2, 3, 3, 3), (2, 3, 4, 3),
          (2, 3, 5, 3), (2, 4, 2, 4), (2, 4, 3, 4), (2, 4, 4, 4), (2, 4, 5, 4), (2, 4, 6, 4), (2, 4, 7, 4), (2, 4, 8, 4), (2, 3, 4, 6),
          (2, 3, 5, 6), (2, 3, 6, 6), (2, 3, 7, 6), (2, 4, 4, 6), (2, 4, 5, 6), (2, 4, 6, 6), (2, 4, 4, 7), (2, 4, 5, 7)]
NSHAPES = len(SHAPES)

STATS_DEFECTS = ('dead_rows_counted', 'last_row_dropped', 'stats_of_rounded_y', 'bias_not_in_stats', 'acc_in_not_in_stats')
ELEMENT_DEFECTS = ('next_utterance_row', 'one_product_dropped')
FUSED_DEFECTS = ('halo_off_by_one', 'mask_before_residual', 'clamp_before_shift', 'res_lo_ignored')
CONV_DEFECTS = STATS_DEFECTS + ELEMENT_DEFECTS + FUSED_DEFECTS


def bf16(x):
    """the nearest bf16 value, as float32"""
    return bf16_to_f32(bf16_rne(np.asarray(x, dtype=np.float32)))


# ---- the convolution ---------------------------------------------------------------------------------------------------------------

def conv_fwd_ref(x, w, bias, Tout, stride, dil, acc_in=None, defect=None, rows=None, x_tail=None):
    """v[n][t][co] = sum_{k,ci} w[co][ci][k] x[n][t*stride + k*dil][ci] + bias[co] (+ acc_in[n][t][co]) as Tr [N][Tout][Cout].
    x [N][per][Cin] (per >= the rows an utterance needs; the operands are the bf16 values exactly as uploaded), w [Cout][Cin][Kw].
    A is the same expression on absolute values, the depth Kw Cin (the dot product) + 1 (bias) (+ 1: acc_in, added last).
    rows (optional): the output rows to evaluate instead of range(Tout) -- rows t >= Tout read on into the rows that follow the
    utterance in memory (x_tail [rows][Cin]: the rows behind the last utterance), stopping at the last row of the buffer (the
    kernel clamps there): what a dead column of a tile holds.
    defect 'next_utterance_row': utterance n starts at n * (the rows it needs), not at n * per;
           'one_product_dropped': the largest of the Kw Cin products of the last element is missing."""
    x = np.asarray(x, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64)
    N, per, Cin = x.shape
    Cout, _, Kw = w.shape
    need = (Tout - 1) * stride + (Kw - 1) * dil + 1
    assert per >= need
    flat = x.reshape(N * per, Cin)
    if x_tail is not None:
        flat = np.concatenate([flat, np.asarray(x_tail, dtype=np.float64)])
    last = len(flat) - 1
    rows = np.arange(Tout) if rows is None else np.asarray(rows)
    ustride = need if defect == 'next_utterance_row' else per
    v = np.zeros((N, len(rows), Cout))
    A = np.zeros((N, len(rows), Cout))
    for n in range(N):
        for k in range(Kw):
            r = np.minimum(n * ustride + rows * stride + k * dil, last)
            win = flat[r]
            v[n] += win @ w[:, :, k].T
            A[n] += np.abs(win) @ np.abs(w[:, :, k]).T
    if defect == 'one_product_dropped':
        win = np.stack([flat[min((N - 1) * per + rows[-1] * stride + k * dil, last)] for k in range(Kw)], axis=1)     # [Cin][Kw]
        term = w[-1] * win
        term = term.reshape(-1)[np.abs(term).argmax()]
        v[-1, -1, -1] -= term
        A[-1, -1, -1] -= abs(term)
    d = Kw * Cin
    if bias is not None:
        b = np.asarray(bias, dtype=np.float64)
        v, A, d = v + b, A + np.abs(b), d + 1
    if acc_in is not None:
        a = np.asarray(acc_in, dtype=np.float64)
        v, A, d = v + a, A + np.abs(a), d + 1
    return Tr(v, A, d)


def stats_sum_depth(shape, N, Tout, slots, launches=1):
    """additions on the longest path of one statistics sum (module docstring), for block shape index `shape` writing slot rows
    (slots > 0; `launches` launches adding onto the same rows) or one row per 128-column tile (slots = 0)"""
    _, nw, _, ns = SHAPES[shape % NSHAPES]
    bn = 16 * nw * ns
    if slots:
        return ns + 4 + nw + -(-(N * -(-Tout // bn)) // slots) * launches
    assert bn in (128, 256)
    return ns + 4 + nw // (bn // 128)


def stats_sum_depth_max(N, Tout, slots=8, launches=1):
    """the deepest chain of any configuration the GPU test forces: the widest bound it ever applies"""
    return max([stats_sum_depth(i, N, Tout, slots, launches) for i in range(NSHAPES)] +
               [stats_sum_depth(i, N, Tout, 0) for i in range(NSHAPES) if 16 * SHAPES[i][1] * SHAPES[i][3] in (128, 256)])


def conv_stats_ref(v, sum_depth=0, defect=None, dead=None, bias=None, acc_in=None):
    """(s1, s2) as Tr [Cout]: the sums over (n, t < Tout) of v and v*v, on the unrounded value.  v: Tr [N][Tout][Cout] (a plain
    array counts as exact: the epilogue-alone form).  sum_depth: stats_sum_depth of the configuration.
    defects: 'dead_rows_counted' (dead: Tr [N][rows][Cout], the values of the rows Tout .. tile end, enter the sums),
    'last_row_dropped' (the last utterance's last row is missing), 'stats_of_rounded_y' (sums of bf16(v)), 'bias_not_in_stats'
    (bias given: sums of v - bias), 'acc_in_not_in_stats' (acc_in given: sums of v - acc_in)"""
    v = v if isinstance(v, Tr) else Tr(v)
    val, a = v.v, v.a
    if defect == 'stats_of_rounded_y':
        val = bf16(val).astype(np.float64)
        a = np.maximum(a, np.abs(val))
    elif defect == 'bias_not_in_stats' and bias is not None:
        val = val - np.asarray(bias, dtype=np.float64)
    elif defect == 'acc_in_not_in_stats' and acc_in is not None:
        val = val - np.asarray(acc_in, dtype=np.float64)
    elif defect == 'last_row_dropped':
        val, a = val.copy(), a.copy()
        val[-1, -1], a[-1, -1] = 0.0, 0.0
    elif defect == 'dead_rows_counted' and dead is not None and dead.v.shape[1] > 0:
        val, a = np.concatenate([val, dead.v], axis=1), np.concatenate([a, dead.a], axis=1)
    t = Tr(val, a, v.d)
    sq = t * t
    return Tr(t.v.sum((0, 1)), t.a.sum((0, 1)), t.d + sum_depth), Tr(sq.v.sum((0, 1)), sq.a.sum((0, 1)), sq.d + sum_depth)


# ---- the fused inference unit ------------------------------------------------------------------------------------------------------

def infer_ref(v, scale, shift, res, res_lo, act, lens, out_rows, pad_l, pad_r, pad_mode, defect=None):
    """The documented sequence of w2l_conv1d_igemm_bnact on v = acc + bias (+ acc_in) (a Tr from conv_fwd_ref, or the fp32 store
    of the plain launch as a plain array: the epilogue-alone form), built on bn_refs.bn_act_fwd_ref with p = 0:
        v * scale + shift;  + res (+ res_lo);  clamp / ReLU;  0 for t >= lens[n];  frame t at row pad_l + t of [N][out_rows][Cout],
        halo rows = the frame they mirror (reflect) or zero, rows beyond pad_l + Tout + pad_r untouched (NaN here).
    Returns dict: a (Tr, padded; round with R_BF16, or R_SPLIT for out_hi + out_lo), src (the frame every row copies, -1: zero),
    written (rows the launch writes).
    The residual sum is ((z + res) + res_lo): two additions, both operands exact -- passed on as ONE tracked operand whose
    magnitude is |res| + |res_lo| and whose depth makes the total depth(z) + 2."""
    v = v if isinstance(v, Tr) else Tr(v)
    N, T, C = v.v.shape
    zd = v.d + (0 if scale is None else 2)
    y2 = None
    if res is not None:
        r = np.asarray(res, dtype=np.float64)
        if res_lo is not None and defect != 'res_lo_ignored':
            lo = np.asarray(res_lo, dtype=np.float64)
            y2 = Tr(r + lo, np.abs(r) + np.abs(lo), zd + 1)
        else:
            y2 = Tr(r)
    y, a = v, act
    if defect == 'clamp_before_shift' and scale is not None:
        y, a = Tr(B.activate(v.v, act), v.a, v.d), 0
    kw = dict(out_rows=out_rows, pad_l=pad_l, pad_r=pad_r, pad_mode=pad_mode)
    out = bn_act_fwd_ref(N, T, C, y, scale, shift, y2=y2, act=a, lens=lens, **kw)
    av, aa, d = out['a'].v.copy(), out['a'].a.copy(), out['a'].d
    src = out['src'].copy()
    if defect == 'mask_before_residual' and y2 is not None and lens is not None:
        late = bn_act_fwd_ref(N, T, C, np.zeros((N, T, C)), None, None, y2=y2, act=act, lens=None, **kw)['a']
        sc = np.where(src >= 0, src, 0)
        for n, lim in enumerate(lens_limits(N, T, lens)):
            masked = (src >= 0) & (sc >= lim)
            av[n, masked], aa[n, masked] = late.v[n, masked], late.a[n, masked]
    if defect == 'halo_off_by_one' and pad_mode == 1:
        halo = (src >= 0) & (np.arange(out_rows) - pad_l != src)
        left = halo & (np.arange(out_rows) < pad_l)
        src2 = np.where(left, src - 1, np.where(halo, src + 1, src))        # the neighbour frame nearer the edge
        prim = pad_l + np.clip(src2, 0, T - 1)
        av, aa = av[:, np.where(halo, prim, np.arange(out_rows))], aa[:, np.where(halo, prim, np.arange(out_rows))]
        src = src2
    written = np.arange(out_rows) < pad_l + T + pad_r
    av[:, ~written] = np.nan
    return dict(a=Tr(av, aa, d), src=src, written=written)


# ---- the cases the CPU and the GPU tests share -------------------------------------------------------------------------------------

@dataclasses.dataclass(frozen=True)
class Fused:
    """one variant of the fused epilogue on a case"""
    name: str
    pad_l: int = 0
    pad_r: int = 0
    pad_mode: int = 0
    act: int = 1
    affine: int = 1       # 0: scale = shift = NULL
    lens: str = 'none'    # 'ragged': a zero, a full length and one in between
    res: int = 0          # 1: res, 2: res and res_lo
    out_lo: int = 0
    acc_in: int = 0
    tail: int = 3         # rows beyond pad_l + Tout + pad_r, never touched


@dataclasses.dataclass(frozen=True)
class ConvCase:
    name: str
    N: int
    Cin: int
    Cout: int
    Kw: int
    stride: int
    dil: int
    Tout: int
    gap: int = 0          # rows between utterances beyond what one needs (x_bstride = (need + gap) Cin)
    fused: tuple = ()
    seed: int = 1

    @property
    def need(self):
        return (self.Tout - 1) * self.stride + (self.Kw - 1) * self.dil + 1

    @property
    def per(self):
        return self.need + self.gap

    @property
    def x_rows_total(self):
        return self.N * self.per + 3          # three more rows than the last utterance's stride: SENTINEL, readable, never needed

    @property
    def K(self):
        return self.Kw * self.Cin


_PAD_A, _PAD_E = (5 - 1) * 2 + 1, (7 - 1) * 1 + 1          # the pad of a consumer one tap longer: odd, so left != right
CONV_A = ConvCase('A_ragged_gap', 3, 64, 192, 5, 1, 2, 141, gap=4, seed=91, fused=(
    Fused('reflect', _PAD_A // 2, _PAD_A - _PAD_A // 2, 1, act=1),
    Fused('reflect_res_lo_out_lo_acc_in', _PAD_A // 2, _PAD_A - _PAD_A // 2, 1, act=2, lens='ragged', res=2, out_lo=1, acc_in=1)))
CONV_B = ConvCase('B_stride2', 2, 64, 128, 11, 2, 1, 77, seed=92, fused=(Fused('reflect_4_5', 4, 5, 1, act=1),))
CONV_C = ConvCase('C_1x1', 5, 192, 64, 1, 1, 1, 97, seed=93, fused=(Fused('dense_act0', act=0, tail=0),))
CONV_D = ConvCase('D_19_columns', 12, 128, 128, 7, 1, 4, 19, seed=94, fused=(
    Fused('zero_ragged_res', 24, 12, 0, act=2, lens='ragged', res=1),))
CONV_E = ConvCase('E_28_steps', 2, 256, 320, 7, 1, 1, 300, seed=95, fused=(
    Fused('reflect', _PAD_E // 2, _PAD_E - _PAD_E // 2, 1, act=2),
    Fused('zero_ragged_res', 3, 7, 0, act=1, lens='ragged', res=1)))
CONV_CASES = [CONV_A, CONV_B, CONV_C, CONV_D, CONV_E]
# E's geometry with 13 utterances: the smallest batch at which several block shapes have eight K steps for each stream-K range,
# so that stream-K really runs (on the five cases above a stream-K index only reaches the fall-back to one block per tile)
CONV_SK = ConvCase('F_stream_k', 13, 256, 320, 7, 1, 1, 300, seed=96)


def conv_lens(kind, N, T):
    if kind == 'none':
        return None
    return np.array(([T, T // 2, 0] + [T - 1 - i for i in range(N)])[:N] if N >= 3 else [T // 2, T][:N], dtype=np.int32)


def make_conv_case(c):
    """operands of a case, every value a bf16 (fp32 for bias / scale / shift / acc_in) value held in float32:
    x [x_rows_total][Cin]: N(0,1) in the rows a live output reads, SENTINEL in every other row (the gap rows between utterances, the
    rows after the last one) -- with zeros there a miscounted dead column could not show; w [Cout][Cin][Kw] N(0,1); bias of
    magnitude 0.5 .. 1.5; acc_in [N][Tout][Cout] fp32 of the output's own magnitude; per fused variant scale ~ 1 / sqrt(Kw Cin)
    (so the unit's output is O(1)), shift N(0,1) with every seventh channel near the clamp's upper edge, res / res_lo, lens."""
    rng = np.random.default_rng(c.seed)
    x = np.full((c.x_rows_total, c.Cin), SENTINEL, dtype=np.float32)
    for n in range(c.N):
        x[n * c.per: n * c.per + c.need] = bf16(rng.standard_normal((c.need, c.Cin)))
    w = bf16(rng.standard_normal((c.Cout, c.Cin, c.Kw)))
    bias = ((0.5 + rng.random(c.Cout)) * np.where(rng.random(c.Cout) < 0.5, -1.0, 1.0)).astype(np.float32)
    acc_in = (rng.standard_normal((c.N, c.Tout, c.Cout)) * np.sqrt(c.K)).astype(np.float32)
    D = dict(x=x, w=w, bias=bias, acc_in=acc_in, fused={})
    for f in c.fused:
        shift = rng.standard_normal(c.Cout)
        shift[::7] += 19.0
        res = bf16(rng.standard_normal((c.N, c.Tout, c.Cout)) * 2) if f.res else None
        D['fused'][f.name] = dict(
            scale=((0.5 + rng.random(c.Cout)) / np.sqrt(c.K)).astype(np.float32) if f.affine else None,
            shift=shift.astype(np.float32) if f.affine else None, res=res,
            res_lo=bf16(rng.standard_normal((c.N, c.Tout, c.Cout)) * 2.0 ** -8) if f.res == 2 else None,
            lens=conv_lens(f.lens, c.N, c.Tout))
    # the lo halves of the three-pass fp32 sequence (hi*hi, hi*lo, lo*hi): bf16 values 2^-8 of the hi operand's size
    D['x_lo'] = np.where(x == SENTINEL, SENTINEL, bf16(rng.standard_normal(x.shape) * 2.0 ** -8)).astype(np.float32)
    D['w_lo'] = bf16(rng.standard_normal(w.shape) * 2.0 ** -8)
    return D


def x_view(c, D):
    """[N][per][Cin] view of the flat operand"""
    return D['x'][:c.N * c.per].reshape(c.N, c.per, c.Cin)


def w_device(D):
    """the kernel's weight layout [Kw][Cout][Cin]"""
    return np.ascontiguousarray(D['w'].transpose(2, 0, 1))


def dead_rows(c):
    """the dead columns of the last 128-column tile of an utterance"""
    return np.arange(c.Tout, -(-c.Tout // 128) * 128)


def conv_ref_of(c, D, defect=None, acc_in=False, sum_depth=None, launches=1, v=None):
    """dict v (Tr [N][Tout][Cout]), s1, s2 (Tr [Cout]) of a case, with the widest chain depth the GPU test applies unless given.
    v: the good convolution, where the caller has it already (a statistics defect leaves it as it is)"""
    acc = D['acc_in'] if acc_in else None
    xd = x_view(c, D)
    if v is None or defect in ELEMENT_DEFECTS:
        v = conv_fwd_ref(xd, D['w'], D['bias'], c.Tout, c.stride, c.dil, acc_in=acc, defect=defect if defect in ELEMENT_DEFECTS else None)
    depth = stats_sum_depth_max(c.N, c.Tout, launches=launches) if sum_depth is None else sum_depth
    dead = None
    if defect == 'dead_rows_counted':
        dead = conv_fwd_ref(xd, D['w'], D['bias'], c.Tout, c.stride, c.dil, rows=dead_rows(c), x_tail=D['x'][c.N * c.per:])
    s1, s2 = conv_stats_ref(v, depth, defect=defect if defect in STATS_DEFECTS else None, dead=dead, bias=D['bias'], acc_in=acc)
    return dict(v=v, s1=s1, s2=s2)


def fused_ref_of(c, D, f, defect=None, src=None):
    """infer_ref of variant f of a case; src: the plain fp32 store (acc + bias) as exact input instead of the float64 convolution"""
    P = D['fused'][f.name]
    acc = D['acc_in'] if f.acc_in else None
    if src is None:
        v = conv_fwd_ref(x_view(c, D), D['w'], D['bias'], c.Tout, c.stride, c.dil, acc_in=acc,
                         defect=defect if defect in ELEMENT_DEFECTS else None)
    else:
        v = Tr(src) if acc is None else Tr(src) + Tr(acc)
    return infer_ref(v, P['scale'], P['shift'], P['res'], P['res_lo'], f.act, P['lens'], f.pad_l + c.Tout + f.pad_r + f.tail,
                     f.pad_l, f.pad_r, f.pad_mode, defect=defect if defect in FUSED_DEFECTS else None)


def dropped_row_over_full_bound(c):
    """what one dropped row is of the FULL bound of s1, in the channel where it shows best, for N(0,1) operands:
        the row's value v is a sum of K = Kw Cin products of unit variance: |v| ~ sqrt(K) z, and over Cout channels the largest |z|
            is about sqrt(2 ln(2 Cout));
        the bound is (K + 1 + chain + 2) u sum A over the R = N Tout rows, A = sum |w||x| ~ K E|w| E|x| = K 2 / pi per element.
    The ratio falls as 1 / (R sqrt(K)): a long K loop or many rows hide a row inside the dot product's share of the bound."""
    K, rows = c.K, c.N * c.Tout
    depth = K + 1 + stats_sum_depth_max(c.N, c.Tout) + 2
    return np.sqrt(K) * np.sqrt(2 * np.log(2 * c.Cout)) / (depth * U * rows * K * 2 / np.pi)


def conv_defect_applies(c, defect, acc_in=False, f=None):
    """can this defect change what a launch of this case (plain: f None; fused variant f) produces?
    dead_rows_counted: Tout is no multiple of 128 (every block shape's last tile then holds dead columns, which read the next
        utterance's rows or SENTINEL rows); bias_not_in_stats, one_product_dropped: always;
    last_row_dropped: always against the EPILOGUE-ALONE bound; against the full bound where dropped_row_over_full_bound() > 1
        (an estimate from the geometry and the operands' distribution: 2.1 on case E, measured 1.6; 0.32 on case F, measured 0.32);
    stats_of_rounded_y: always -- but only the EPILOGUE-ALONE bound shows it (on B, D and E the rounding of 16 000 values averages
        out below the dot product's share of the full bound), so it is asserted against that bound alone;
    acc_in_not_in_stats: launches with accumulate = 1; next_utterance_row: utterances further apart than their rows, N > 1;
    the fused four: reflect pads; ragged lens with a residual operand; an activation with an affine map; a res_lo operand."""
    if defect in STATS_DEFECTS and f is not None:
        return False
    if defect == 'dead_rows_counted':
        return c.Tout % 128 != 0
    if defect == 'last_row_dropped':
        return dropped_row_over_full_bound(c) > 1
    if defect == 'acc_in_not_in_stats':
        return acc_in
    if defect == 'next_utterance_row':
        return c.gap > 0 and c.N > 1
    if defect in FUSED_DEFECTS and f is None:
        return False
    if defect == 'halo_off_by_one':
        return f.pad_mode == 1 and f.pad_l + f.pad_r > 0
    if defect == 'mask_before_residual':
        return f.lens == 'ragged' and f.res > 0
    if defect == 'clamp_before_shift':
        return f.act != 0 and f.affine == 1
    if defect == 'res_lo_ignored':
        return f.res == 2
    return True


# launches of the GPU sweep over case E (every fifth index from 52 on) that w2l_conv_plan says really split / really run stream-K
# with the full workspace: what the geometry yields (tests/test_cpu_conv_refs.py recomputes it with the host-only plan query)
# (60 of its 73 indices split; none runs stream-K: 18 tiles x 28 steps is far below eight steps for each of 512 ranges, so on these
# shapes a stream-K index only exercises the documented fall-back to one block per tile)
E_SPLIT_FLOOR, E_STREAMK_FLOOR = 60, 0
# case F: the stream-K indices whose plan has stream-K blocks, slot rows (24) plus tile rows on 128 / 256 columns (14)
SK_FLOOR = 38
