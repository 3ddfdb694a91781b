"""Float64 restatement of the sample-rate converter, written from its definition -- plain NumPy, nothing of the package:

    P/Q = input samples advanced per output sample (reduced);  n_out = ceil(n_in Q / P);
    out[m] = sum_{j < K} x~[i0 - H + j] h[phase][j],  i0 = (m P) div Q,  phase = (m P) mod Q  (int64),  x~ = 0 outside [0, n_in)
    c = rolloff min(1, Q/P),  W = Z / c,  H = ceil(W),  K = 2H + 2,  u = (j - H) - p/Q,
    h[p][j] = c sinc(c u) I0(beta sqrt(1 - (u/W)^2)) / I0(beta)  for |u| < W, else 0;   Z = 16, beta = 9, rolloff = 0.92.

The bound is kernel_refs' dot-product rule: K fp32 products summed in any order, |got - ref| <= (K + 2) 2^-24 sum_j |x~ h|.
"""
import math

import numpy as np

from kernel_refs import dot_bound

Z, BETA, ROLLOFF = 16, 9.0, 0.92


def n_out_ref(n_in, P, Q):
    return (n_in * Q + P - 1) // P


def bank_ref(P, Q, zeros=Z, beta=BETA, rolloff=ROLLOFF, phases=None):
    """(float64 [Q][K], H), element by element; ``phases``: fill only these rows (the others stay zero)"""
    c = rolloff * min(1.0, Q / P)
    W = zeros / c
    H = int(math.ceil(W))
    K = 2 * H + 2
    h = np.zeros((Q, K), dtype=np.float64)
    i0b = float(np.i0(beta))
    for p in (range(Q) if phases is None else phases):
        for j in range(K):
            u = (j - H) - p / Q
            if abs(u) < W:
                t = u / W
                h[p, j] = c * float(np.sinc(c * u)) * float(np.i0(beta * math.sqrt(1.0 - t * t))) / i0b
    return h, H


def resample_ref(x, P, Q, bank_fp32, m_lo=0, m_hi=None):
    """outputs m_lo <= m < m_hi (default: all n_out) of row x through the fp32 bank, in float64.  Returns (ref, A) with
    A = sum_j |x~ h| per output; the dot product has K terms."""
    x = np.asarray(x, dtype=np.float64)
    h = np.asarray(bank_fp32, dtype=np.float64)
    n_in = x.shape[0]
    Qb, K = h.shape
    assert Qb == Q and K % 2 == 0
    H = (K - 2) // 2
    m_hi = n_out_ref(n_in, P, Q) if m_hi is None else m_hi
    m = np.arange(m_lo, m_hi, dtype=np.int64)
    pos = m * np.int64(P)
    i0 = pos // np.int64(Q)
    phase = pos - i0 * np.int64(Q)
    idx = (i0 - H)[:, None] + np.arange(K, dtype=np.int64)[None, :]
    ok = (idx >= 0) & (idx < n_in)
    xt = np.where(ok, x[np.clip(idx, 0, max(n_in - 1, 0))], 0.0)
    prod = xt * h[phase]
    return prod.sum(axis=1), np.abs(prod).sum(axis=1)


def resample_bound(A, K, ref):
    return dot_bound(A, K, ref)
