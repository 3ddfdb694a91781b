"""Float64 references of the depthwise-convolution, fused-optimizer and pad-cast kernels, restated from the formulas in
csrc/dwconv.hip, csrc/pack.hip, csrc/optim.hip and csrc/common.h -- plain NumPy, nothing of the engine's Python.

Every reference returns the exact result (the inputs are fp32 / bf16 values, so float64 holds every product exactly and
the sums to ~1e-16) AND what the error bound of the fp32 device kernel needs.

The bound.  With u = 2^-24 (fp32 unit roundoff), a value the device computes through a tree of fp32 operations obeys

    |got - ref| <= gamma_d * A,      gamma_d = d u / (1 - d u) <= (d + 2) u   for d < 5000,

where A is the same expression evaluated on absolute values ("the magnitude sum", A = sum |term| for a dot product) and d
counts the roundings on the longest path from an input to the result.  The rules, each one line of (1 + delta) algebra:
    x + y, x - y :  A = A_x + A_y,  d = max(d_x, d_y) + 1       (both inputs exact: one rounding of the result, A = |x + y|)
    x * y, x / y :  A = A_x * A_y (A_x / |y|),  d = d_x + d_y + 1    (y of a quotient must be free of cancellation: A_y = |y|)
    sqrt(x)      :  x free of cancellation;  A = sqrt(x), d = d_x + 1   (sqrt halves a relative error)
    clamp, max   :  1-Lipschitz: A and d pass through unchanged
An FMA contraction only removes roundings; any summation order of n terms takes one term through at most n - 1 additions
that round (adding an exact zero does not), so a dot product of n terms has d = n: the issue's (n_terms + 2) u A.
On top comes the rounding into the output format, r_out: 0 for fp32, 2^-8 |ref| for bf16 (RNE: half an ulp of 8
significand bits), 2^-17 |ref| for a hi+lo pair (csrc/common.h).  ``Tr`` below carries (v, a, d) through these rules.
"""
import numpy as np

U = 2.0 ** -24
R_BF16 = 2.0 ** -8
R_SPLIT = 2.0 ** -17


# ---- bf16 at the bit level --------------------------------------------------------------------------------------------

def bf16_rne(x):
    """fp32 -> bf16 bits (uint16), round to nearest, ties to even; NaN stays a (quiet) NaN, overflow goes to inf"""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    r = ((b.astype(np.uint64) + 0x7FFF + ((b >> 16) & 1)) >> 16).astype(np.uint16)
    nan = (b & 0x7FFFFFFF) > 0x7F800000
    return np.where(nan, ((b >> 16) | 0x0040).astype(np.uint16), r)


def bf16_to_f32(bits):
    return (np.ascontiguousarray(bits, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


def split_bf16(x):
    """common.h f32_split_bf16: hi = bf16(f), lo = bf16(f - hi), the difference taken in fp32 (it is exact there)"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    hi = bf16_rne(x)
    with np.errstate(invalid='ignore'):
        lo = bf16_rne((x - bf16_to_f32(hi)).astype(np.float32))
    return hi, lo


# ---- tracked values: exact value, magnitude sum, rounding depth -------------------------------------------------------------

class Tr:
    """v: exact value (float64), a: the expression on absolute values (>= |v|), d: roundings on the longest path"""

    def __init__(self, v, a=None, d=0):
        self.v = np.asarray(v, dtype=np.float64)
        self.a = np.abs(self.v) if a is None else np.asarray(a, dtype=np.float64)
        self.d = int(d)

    def __add__(self, o):
        if self.d == 0 and o.d == 0:           # two exact inputs: one rounding, relative to the RESULT
            return Tr(self.v + o.v, None, 1)
        return Tr(self.v + o.v, self.a + o.a, max(self.d, o.d) + 1)

    def __sub__(self, o):
        if self.d == 0 and o.d == 0:
            return Tr(self.v - o.v, None, 1)
        return Tr(self.v - o.v, self.a + o.a, max(self.d, o.d) + 1)

    def __mul__(self, o):
        return Tr(self.v * o.v, self.a * o.a, self.d + o.d + 1)

    def __truediv__(self, o):
        assert np.array_equal(o.a, np.abs(o.v)), 'divisor with cancellation'
        return Tr(self.v / o.v, self.a / o.a, self.d + o.d + 1)

    def sqrt(self):
        assert np.array_equal(self.a, np.abs(self.v)) and (self.v >= 0).all()
        return Tr(np.sqrt(self.v), None, self.d + 1)

    def bound(self, r_out=0.0):
        """per-element bound of |device - v| for an output format with relative rounding r_out"""
        assert self.d < 5000
        return (self.d + 2) * U * self.a + r_out * np.abs(self.v)


def f32(x):
    """a scalar as the C ABI receives it (float), exactly, in float64"""
    return float(np.float32(x))


def dot_bound(A, n_terms, ref, r_out=0.0):
    """(n_terms + 2) u A + r_out |ref|"""
    return (n_terms + 2) * U * np.asarray(A, dtype=np.float64) + r_out * np.abs(ref)


# ---- depthwise convolution (csrc/dwconv.hip) ---------------------------------------------------------------------------------

def _lims(N, Tout, lens):
    if lens is None:
        return [Tout] * N
    return [max(0, min(Tout, int(l))) for l in lens]


def dw_fwd_ref(xp, w, N, Tout, C, K, s, d, lens):
    """y[n][t][c] = sum_k w[k][c] * xp[n][t*s + k*d][c]; rows t >= lens[n] are zero.  xp [N][x_rows][C], w [K][C].
    Returns (y, A) with A = sum_k |w| |xp|; n_terms = K."""
    xp = np.asarray(xp, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64)
    y = np.zeros((N, Tout, C))
    A = np.zeros((N, Tout, C))
    for k in range(K):
        win = xp[:, k * d: k * d + (Tout - 1) * s + 1: s, :]
        y += w[k] * win
        A += np.abs(w[k]) * np.abs(win)
    for n, lim in enumerate(_lims(N, Tout, lens)):
        y[n, lim:] = 0.0
        A[n, lim:] = 0.0
    return y, A


def dw_dgrad_ref(dy, w, N, Tp, Tout, C, K, d, lens):
    """dxp[n][v][c] = sum_k w[k][c] * dy[n][v - k*d][c] (stride 1); dy rows outside [0, min(Tout, lens[n])) count as zero.
    dy [N][dy_rows >= Tout][C].  Returns (dxp [N][Tp][C], A); n_terms = K."""
    dy = np.asarray(dy, dtype=np.float64)[:, :Tout].copy()
    w = np.asarray(w, dtype=np.float64)
    for n, lim in enumerate(_lims(N, Tout, lens)):
        dy[n, lim:] = 0.0
    dx = np.zeros((N, Tp, C))
    A = np.zeros((N, Tp, C))
    for k in range(K):
        L = min(Tout, Tp - k * d)
        if L <= 0:
            break
        dx[:, k * d: k * d + L] += w[k] * dy[:, :L]
        A[:, k * d: k * d + L] += np.abs(w[k]) * np.abs(dy[:, :L])
    return dx, A


def dw_wgrad_ref(dy, xp, N, Tout, C, K, s, d, lens):
    """dw[k][c] = sum_{n, t < min(Tout, lens[n])} dy[n][t][c] * xp[n][t*s + k*d][c].
    Returns (dw [K][C], A [K][C], n_terms) with n_terms = the number of valid (n, t) rows."""
    dy = np.asarray(dy, dtype=np.float64)[:, :Tout].copy()
    xp = np.asarray(xp, dtype=np.float64)
    lims = _lims(N, Tout, lens)
    for n, lim in enumerate(lims):
        dy[n, lim:] = 0.0
    dw = np.zeros((K, C))
    A = np.zeros((K, C))
    for k in range(K):
        win = xp[:, k * d: k * d + (Tout - 1) * s + 1: s, :]
        dw[k] = (dy * win).sum(axis=(0, 1))
        A[k] = (np.abs(dy) * np.abs(win)).sum(axis=(0, 1))
    return dw, A, int(sum(lims))


# ---- SGD (csrc/optim.hip sgd_pack_kernel, sgd_small_multi_kernel) ------------------------------------------------------------

def sgd_ref(p, g, m, first, lr, mu, wd, nesterov, coef=None, bound=None):
    """torch.optim.SGD, dampening 0:  g' = clamp(g*coef, -bound, bound) (only if coef is given) + wd*p;
    m' = g' on the first step, else mu*m + g';  p' = p - lr*(nesterov ? g' + mu*m' : m').  m = None: no momentum buffer
    (torch's momentum = 0): p' = p - lr*g'.  NaN stays NaN.  Returns (p', m') as Tr (m' is None without a buffer)."""
    lr, mu, wd = Tr(f32(lr)), Tr(f32(mu)), Tr(f32(wd))
    P = Tr(p)
    G = Tr(g)
    if coef is not None:
        G = G * Tr(f32(coef))
        b = f32(bound)
        with np.errstate(invalid='ignore'):
            v = np.where(G.v < -b, -b, G.v)
            v = np.where(v > b, b, v)
        G = Tr(v, G.a, G.d)
    if wd.v != 0:
        G = G + wd * P
    if m is None:
        return P - lr * G, None
    M = G if first else mu * Tr(m) + G
    step = (G + mu * M) if nesterov else M
    return P - lr * step, M


# ---- Novograd (csrc/optim.hip) -------------------------------------------------------------------------------------------------

def novograd_norm_depth(n, nblocks):
    """roundings on the longest path of ||g||^2: the square, a thread's chain of additions over its strided share, the
    256-wide tree (8 levels), the finalize thread's chain over its share of the partials, the second tree"""
    per_thread = -(-n // (nblocks * 256))
    return 1 + per_thread + 8 + -(-nblocks // 256) + 8


def novograd_nblocks(n, scratch_floats):
    """the host's choice of the number of partial sums: ~16 elements per thread, at most scratch_floats - 1 and 1024"""
    return max(1, min((n + 4095) // 4096, scratch_floats - 1, 1024))


def novograd_ref(p, g, m, v, vmax, lr, b1, b2, eps, wd, grad_averaging, norm_depth=0):
    """norm = ||g||^2;  v' = norm if v == 0 else b2*v + (1-b2)*norm;  amsgrad (vmax given): vmax' = max(vmax, v'), used for
    the denominator;  g' = g/(sqrt(v')+eps) + wd*p;  g' *= (1-b1) if grad_averaging;  m' = b1*m + g';  p' = p - lr*m'.
    Returns (p', m', v', vmax') as Tr (vmax' None without amsgrad)."""
    g64 = np.asarray(g, dtype=np.float64)
    one = Tr(1.0)
    B1, B2 = Tr(f32(b1)), Tr(f32(b2))
    norm = Tr(float((g64 * g64).sum()), None, norm_depth)
    V = norm if float(v) == 0.0 else B2 * Tr(float(v)) + (one - B2) * norm
    VM = None
    used = V
    if vmax is not None:
        VM = Tr(max(float(vmax), float(V.v)), None, V.d)
        used = VM
    denom = used.sqrt() + Tr(f32(eps))
    G = Tr(g64) / denom
    P = Tr(p)
    if f32(wd) != 0:
        G = G + Tr(f32(wd)) * P
    if grad_averaging:
        G = G * (one - B1)
    M = B1 * Tr(m) + G
    return P - Tr(f32(lr)) * M, M, V, VM


# ---- classifier-gradient layout (csrc/pack.hip pad_cast_kernel, colsum_kernel) -----------------------------------------------------

def pad_cast_ref(g, N, T, C, CP, halo):
    """dense [N][T][C] -> shared-halo [halo + N*(T+halo)][CP]: row halo + n*(T+halo) + t holds frame (n, t), every other
    row and every column c >= C is zero.  Returns (layout, colsum [CP], A [CP]); colsum has n_terms = N*T."""
    g = np.asarray(g, dtype=np.float64).reshape(N, T, C)
    out = np.zeros((halo + N * (T + halo), CP))
    for n in range(N):
        r = halo + n * (T + halo)
        out[r: r + T, :C] = g[n]
    cs = np.zeros(CP)
    A = np.zeros(CP)
    cs[:C] = g.sum(axis=(0, 1))
    A[:C] = np.abs(g).sum(axis=(0, 1))
    return out, cs, A


# ---- the cases the CPU and the GPU tests share ------------------------------------------------------------------------------

# (N, Tout, C, K, stride, dil).  The fifth: N*Tout*(C/8) = 3*5462*128 = 2 097 408 items = 8193 blocks of 256 > the 8192-block
# cap (Tout = 5461 gives exactly 8192), so the grid-stride loop of dw_fwd / dw_dgrad runs a second round.
DW_SHAPES = [(2, 37, 8, 1, 1, 1), (3, 301, 96, 13, 1, 2), (2, 130, 40, 11, 2, 1), (2, 65, 2048, 33, 1, 1),
             (3, 5462, 1024, 5, 1, 1), (2, 75, 256, 75, 1, 1)]
LENS_KINDS = ('none', 'full', 'ragged', 'over')


def dw_lens(kind, N, Tout):
    """null; all-full; [Tout, Tout//2, 0]-style (a zero included); a value above Tout"""
    if kind == 'none':
        return None
    if kind == 'full':
        return np.full(N, Tout, dtype=np.int32)
    if kind == 'ragged':
        return np.array(([Tout, Tout // 2, 0] if N >= 3 else [Tout // 2, 0])[:N], dtype=np.int32)
    return np.array(([Tout + 5, Tout - 3, Tout + 1000])[:N], dtype=np.int32)


# (first, nesterov, wd, zero_grad, lo operands, e4m3 operands): every pair of values of any two flags occurs
SGD_FLAG_SETS = [(0, 0, 0.0, 0, 0, 0), (0, 0, 1e-3, 1, 1, 1), (0, 1, 0.0, 1, 0, 1), (0, 1, 1e-3, 0, 1, 0),
                 (1, 0, 0.0, 1, 1, 0), (1, 0, 1e-3, 0, 0, 1), (1, 1, 0.0, 0, 1, 1), (1, 1, 1e-3, 1, 0, 0),
                 (0, 0, 0.0, 0, 1, 1), (1, 1, 1e-3, 1, 1, 1), (0, 1, 1e-3, 1, 0, 0), (1, 0, 0.0, 0, 0, 0)]
# (coef, bound) of the _clip entry points: identity, norm mode, value mode
SGD_CLIPS = [(1.0, float('inf')), (0.37, float('inf')), (1.0, 0.01)]
SGD_LR, SGD_MU = 0.05, 0.9
