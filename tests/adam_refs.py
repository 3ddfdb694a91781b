"""Float64 reference of the fused Adam / AdamW kernels (csrc/optim.hip: adam_update, adam_pack_kernel,
adam_small_multi_kernel, adam_tick_kernel), restated from their formulas with kernel_refs.Tr -- plain NumPy.

The rule, in torch's order (_single_tensor_adam; amsgrad, maximize off), with the three step-dependent scalars
dyn = [lr, lr / (1 - beta1^t), sqrt(1 - beta2^t)] as the device holds them (fp32 values, taken as exact inputs):

    g' = clamp(g*coef, -bound, bound)                (only with a clip)
    decoupled:  p1 = p * (1 - dyn0*wd)               else:  g' = g' + wd*p,  p1 = p
    m' = beta1*m + (1-beta1)*g'      v' = beta2*v + (1-beta2)*g'*g'
    p' = p1 - dyn1 * m' / (sqrt(v')/dyn2 + eps)

The bound.  m' and v' are sums of products: kernel_refs.Tr carries (value, magnitude sum, rounding depth) through them and
Tr.bound() is their bound, exactly as for sgd_ref.  p1 likewise.  The quotient needs one more step, because Tr's rules for
sqrt and '/' demand an argument free of cancellation and v' has none of that guarantee once g' = g + wd*p cancels: with
e_v = V.bound() and e_m = M.bound() the device's v' lies in [max(v' - e_v, 0), v' + e_v] and its m' in [m' - e_m, m' + e_m];
sqrt, the division by dyn2 and the addition of eps are monotone and each rounds once (correctly rounded fp32: relative u), so
the device's denominator lies in [D_lo, D_hi] = [D(v_lo) (1 - 4u), D(v_hi) (1 + 4u)] (three roundings, one to spare).  The
quotient of two intervals with a positive divisor takes its extremes at the corners; the device's dyn1 * (m'/D), in either
association, adds two roundings of a magnitude <= dyn1 (|m'| + e_m) / D_lo (3u, one to spare); the final subtraction rounds
once more, relative to its own result.  Where nothing cancels the corner bound is the first-order Tr bound to within u^2.
"""
import numpy as np

from kernel_refs import Tr, U, f32


class Bounded:
    """a reference value with a per-element bound computed directly (where Tr's linear rules do not apply)"""

    def __init__(self, v, b):
        self.v, self.b = np.asarray(v, dtype=np.float64), np.asarray(b, dtype=np.float64)

    def bound(self):
        return self.b


def tick_host(n, lr, beta1, beta2):
    """n calls of w2l_adam_tick on a fresh state {0, 1.0, 1.0}, the same double multiplies in the same order ->
    (step, pow1, pow2, [lr, lr / (1 - pow1), sqrt(1 - pow2)] in float64, before the one rounding to fp32)"""
    pow1 = pow2 = 1.0
    for _ in range(n):
        pow1 *= float(beta1)
        pow2 *= float(beta2)
    return n, pow1, pow2, [float(lr), float(lr) / (1.0 - pow1), float(np.sqrt(1.0 - pow2))]


def adam_ref(p, g, m, v, dyn, beta1, beta2, eps, wd, decoupled, coef=None, bound=None, torch_scalars=False):
    """-> (p' as Bounded, m' as Tr, v' as Tr).  ``dyn``: the three scalars as given (the device tests pass the device's own
    fp32 values; the torch pin passes float64 ones); betas, eps, wd are taken as the C ABI receives them (float): the kernels
    form 1 - beta from the FLOAT beta, so the two weights of each moving average sum to one exactly.
    ``torch_scalars``: the weights as torch's own fp32 ops apply them instead -- 1 - beta formed in double from the Python
    float and rounded to fp32 on its own (f32(1 - 0.999) differs from 1 - f32(0.999) by 1.3e-5 relative), the first moment
    as lerp(m, g, w) = (1 - w) m + w g -- for parameters optim.FusedAdamW leaves to torch ops."""
    one = Tr(1.0)
    B1, B2, EPS, WD = Tr(f32(beta1)), Tr(f32(beta2)), f32(eps), Tr(f32(wd))
    OMB1, OMB2 = one - B1, one - B2
    if torch_scalars:
        OMB1, OMB2 = Tr(f32(1.0 - float(beta1))), Tr(f32(1.0 - float(beta2)))
        B1 = Tr(1.0 - OMB1.v)
    d0, d1, d2 = (float(x) for x in dyn[:3])
    P0, G = Tr(p), Tr(g)
    if coef is not None:
        G = G * Tr(f32(coef))
        b = f32(bound)
        with np.errstate(invalid='ignore'):
            x = np.where(G.v < -b, -b, G.v)
            x = np.where(x > b, b, x)
        G = Tr(x, G.a, G.d)
    if decoupled:
        P1 = P0 * (one - Tr(d0) * WD)
    else:
        P1 = P0
        if WD.v != 0:
            G = G + WD * P0
    M = B1 * Tr(m) + OMB1 * G
    V = B2 * Tr(v) + OMB2 * (G * G)
    e_m, e_v = M.bound(), V.bound()

    def denom(x, k):
        return (np.sqrt(x) / d2 + EPS) * (1.0 + k * U)

    D, D_lo, D_hi = denom(V.v, 0), denom(np.maximum(V.v - e_v, 0.0), -4), denom(V.v + e_v, 4)
    q = M.v / D
    corners = [(M.v + sm * e_m) / dd for sm in (-1, 1) for dd in (D_lo, D_hi)]
    e_q = np.max([np.abs(c - q) for c in corners], axis=0)
    big = (np.abs(M.v) + e_m) / D_lo
    upd = d1 * q
    e_upd = abs(d1) * (e_q + 3 * U * big)
    pv = P1.v - upd
    e_p = P1.bound() + e_upd + U * (np.abs(P1.v) + P1.bound() + np.abs(upd) + e_upd)
    return Bounded(pv, e_p), M, V


ADAM_BETAS = (0.9, 0.999)
ADAM_EPS = 1e-8
