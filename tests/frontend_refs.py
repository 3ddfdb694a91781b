"""Float64 references of the feature front-end (csrc/features.hip) and of the softmax / CTC / argmax kernels (csrc/ctc.hip),
restated from the formulas in those two files and from the comments in include/w2l_hip.h -- plain NumPy, nothing of the package's
Python and nothing of oracle/.  Every reference returns the exact value AND a per-element bound of what the fp32 device kernel
may differ by, derived with the rules at the top of kernel_refs.py (u = 2^-24; a result reached through d roundings obeys
|got - ref| <= (d + 2) u A, A the expression on absolute values).  A function call of k ulp counts as 2k roundings of its result
(1 ulp <= 2^-23 |value| = 2u |value|).

Every reference takes ``defect=``: a named, deliberate fault that models a kernel bug.  test_cpu_frontend_refs.py shows that each
one pushes the error / bound ratio above 1 on a case the GPU tests run.
"""
import dataclasses
import functools
import math

import numpy as np

from kernel_refs import U, Tr, dot_bound, f32

# ---- transcendental constants, in ulp: the only numbers here that are taken from documentation and not derived ---------------
LIBM_EXPF = 2         # ROCm device-libs (ocml) expf: documented 1 ulp; the issue's starting value of 2 kept
LIBM_LOGF = 2         # ocml logf: documented 1 ulp; 2 kept
LIBM_LOG1PF = 2       # ocml log1pf: documented 2 ulp
LIBM_SINCOSPIF = 2    # ocml sincospif: documented 2 ulp (1 for sinpi / cospi alone)
LIBM_SQRTF = 2        # sqrtf: correctly rounded (0.5 ulp) under hipcc's default -fhip-fp32-correctly-rounded-divide-sqrt; 2 kept
HW_EXP = 1            # v_exp_f32: 1 ulp (CDNA ISA guide, "transcendental accuracy"); behind __expf(x) = v_exp_f32(x * log2e)
HW_LOG = 1            # v_log_f32: 1 ulp (same table); behind __logf(x) = v_log_f32(x) * ln2
# __expf(x), x <= 0: the argument x*log2e carries the rounding of the product and of the constant, 2u |x| absolute in units of
# ln2, so e^x is off by e^x (2 HW_EXP u + 2u |x|) <= u (2 HW_EXP + 2/e) because |x| e^x <= 1/e.
HW_EXPF_ABS = 2 * HW_EXP + 2 / math.e
# __logf(y), 1 <= y <= 3: v_log_f32 2 HW_LOG u log2(y), then the product with ln2 (its rounding and the constant's): 2u more,
# all relative to ln(y) <= ln 3.
HW_LOGF_ABS = (2 * HW_LOG + 2) * math.log(3.0)
TINY = 2.0 ** -126    # flush-to-zero of a subnormal result


def split_nonfinite(got, ref):
    """elements whose reference is inf / NaN must match exactly (NaN == NaN); returns (ok, got', ref') with those set to 0"""
    got = np.asarray(got, dtype=np.float64)
    nf = ~np.isfinite(ref)
    ok = bool(np.array_equal(got[nf], ref[nf], equal_nan=True))
    return ok, np.where(nf, 0.0, got), np.where(nf, 0.0, ref)


# ---- log-mel (features.hip logmel_kernel, logmel512_kernel) ---------------------------------------------------------------------

def hann(win_length):
    i = np.arange(win_length, dtype=np.float64)
    return (0.5 - 0.5 * np.cos(2 * np.pi * i / win_length)).astype(np.float32)


def filterbank(n_fft, n_mels):
    """triangles on a mel-like (log-spaced above 1/8 of the band) axis over bins -1 .. n_bins, so that DC and the Nyquist bin carry
    weight.  Returns fbT [n_bins][n_mels] fp32 and fb_range [n_mels][2] int32 (first / one-past-last non-zero bin)"""
    nb = n_fft // 2 + 1
    edges = (nb / 8.0) * np.expm1(np.linspace(np.log1p(-8.0 / nb), np.log1p(8.0), n_mels + 2))      # bin -1 .. bin n_bins
    k = np.arange(nb, dtype=np.float64)[:, None]
    lo, ce, hi = edges[None, :-2], edges[None, 1:-1], edges[None, 2:]
    fb = np.maximum(0.0, np.minimum((k - lo) / (ce - lo), (hi - k) / (hi - ce))).astype(np.float32)
    rng = np.zeros((n_mels, 2), dtype=np.int32)
    for m in range(n_mels):
        nz = np.nonzero(fb[:, m])[0]
        if len(nz):
            assert nz[-1] - nz[0] + 1 == len(nz)
            rng[m] = (nz[0], nz[-1] + 1)
    return fb, rng


def fft_const(n_fft):
    """C with |re/im error of a bin| <= C u sum_i |x_i w_i|, the error of the windowed samples themselves aside.
    The error is carried as a complex modulus (a rotation keeps it), one rounding of a component at magnitude <= A (A the
    magnitude sum of the butterfly's subtree) moves the modulus by <= sqrt2 u A.
    radix 2 (logmel_kernel), per stage: twiddle c1 = 2 LIBM_SINCOSPIF (its argument -2k/n is exact), c*xr - sn*xi two
    roundings on a path with |c xr| + |sn xi| <= |x|, the butterfly's add one: sqrt2 (3 + 2 LIBM_SINCOSPIF) per stage, c2 = 0.
    8x8x8 (logmel512_kernel): a dft8 is three add levels plus, on its longest path, the add inside t1/t3, the product with R and
    R's own rounding: 6; a twiddle product is 2 + 2 LIBM_SINCOSPIF (the sign flip of W^(m+256) is exact); three dft8 and two
    twiddle products."""
    if n_fft == 512:
        return math.sqrt(2.0) * (3 * 6 + 2 * (2 + 2 * LIBM_SINCOSPIF))
    return math.sqrt(2.0) * (3 + 2 * LIBM_SINCOSPIF) * int(math.log2(n_fft))


def _reflect(j, L, defect):
    j = np.asarray(j)
    if defect == 'reflect_edge':                      # mirror that repeats the edge sample
        j = np.where(j < 0, -j - 1, j)
        j = np.where(j >= L, 2 * L - 1 - j, j)
    else:
        j = np.where(j < 0, -j, j)
        j = np.where(j >= L, 2 * (L - 1) - j, j)
    return np.clip(j, 0, L - 1)


def logmel_ref(audio, n_samples, noise, dither, preemph, window, n_fft, hop, fbT, fb_range, guard, Tmax, defect=None):
    """audio / noise [N][stride] fp32 (noise may be None), window [win_length], fbT [n_bins][n_mels], fb_range or None.
    Returns (power, power_bound, log, log_bound), each [N][Tmax][n_mels]: the take_log = 0 and take_log = 1 outputs."""
    N = len(n_samples)
    win = len(window)
    nb = n_fft // 2 + 1
    n_mels = fbT.shape[1]
    fb = np.asarray(fbT, dtype=np.float64)
    woff = 0 if defect == 'woff0' else (n_fft - win) // 2
    wfull = np.zeros(n_fft)
    wfull[woff: woff + win] = window
    g = f32(guard)
    P = np.zeros((N, Tmax, n_mels))
    Pb = np.zeros_like(P)
    Lg = np.zeros_like(P)
    Lb = np.zeros_like(P)
    if fb_range is None:
        runs = [(0, nb)] * n_mels
    else:
        runs = [(int(a), int(b) - (1 if defect == 'filter_short' and b > a else 0)) for a, b in fb_range]
    run_len = np.array([max(int((fb[a:b, m] != 0).sum()), 1) for m, (a, b) in enumerate(runs)])
    fbm = np.zeros_like(fb)
    for m, (a, b) in enumerate(runs):
        fbm[a:b, m] = fb[a:b, m]
    for n in range(N):
        L = int(n_samples[n])
        X = Tr(audio[n, :L])
        if noise is not None:
            X = X + Tr(noise[n, :L]) * Tr(f32(dither))
        prev = Tr(np.concatenate([[X.v[-1] if defect == 'preemph_wrap' else 0.0], X.v[:-1]]),
                  np.concatenate([[X.a[-1] if defect == 'preemph_wrap' else 0.0], X.a[:-1]]), X.d)
        Y = X - Tr(f32(preemph)) * prev               # y[0] = x[0]: the subtracted term is an exact zero there
        T_n = (L // hop) if defect == 'frames_L_over_hop' else 1 + L // hop
        live = min(T_n, Tmax)
        if live <= 0:
            continue
        idx = _reflect(np.arange(live)[:, None] * hop - n_fft // 2 + np.arange(n_fft)[None, :], L, defect)
        v = Y.v[idx] * wfull
        a = Y.a[idx] * np.abs(wfull)
        d_v = Y.d + 1
        sumA = a.sum(axis=1)
        e = ((fft_const(n_fft) + d_v + 2) * U * sumA)[:, None]          # re / im error of every bin of the frame
        F = np.fft.rfft(v, axis=1)
        if defect == 'twiddle_sign':                  # -W^1 in the last radix-2 stage: bin 1 becomes X[1 + n/2] = conj X[n/2 - 1]
            F[:, 1] = np.conj(F[:, n_fft // 2 - 1])
        if defect == 'no_nyquist':
            F[:, nb - 1] = 0.0
        pw = F.real ** 2 + F.imag ** 2
        # re^2 + im^2: 2u relative on a path, halved by the root; sqrtf 2 LIBM_SQRTF u; the square doubles and rounds once more
        pwb = 2 * (np.abs(F.real) + np.abs(F.imag)) * e + 2 * e * e + (3 + 4 * LIBM_SQRTF) * U * pw
        mel = pw @ fbm
        melb = pwb @ fbm + dot_bound(mel, run_len[None, :], mel)
        if defect == 'last_frame_zero':
            mel[live - 1] = 0.0
        P[n, :live] = mel
        Pb[n, :live] = melb
        arg = mel + g
        with np.errstate(divide='ignore'):
            lg = np.log(arg) if defect == 'log_not_log1p' else np.log1p(arg)
        if defect == 'last_frame_zero':
            lg[live - 1] = 0.0
        Lg[n, :live] = lg
        Lb[n, :live] = (melb + U * arg) / (1.0 + arg) + 2 * LIBM_LOG1PF * U * np.abs(lg) + TINY
    return P, Pb, Lg, Lb


# ---- per-feature normalisation (features.hip feature_stats_kernel, feature_apply_kernel) -----------------------------------------

STAT_WAVES = 16


def feature_normalize_ref(logmel, n_samples, hop, Tmax, eps, defect=None):
    """logmel [N][Tmax][n_mels] (frames past an utterance's own are never read).  Returns (out [N][n_mels][Tmax], out_bound,
    mean [N][n_mels], mean_bound, std, std_bound).  T_n == 1: std and the utterance's one frame are NaN (bounds 0)."""
    x = np.asarray(logmel, dtype=np.float64)
    N, _, n_mels = x.shape
    out = np.zeros((N, n_mels, Tmax))
    outb = np.zeros_like(out)
    mean = np.zeros((N, n_mels))
    meanb = np.zeros_like(mean)
    std = np.zeros_like(mean)
    stdb = np.zeros_like(mean)
    e = f32(eps)
    for n in range(N):
        T_n = min(1 + int(n_samples[n]) // hop, Tmax)
        Ts = Tmax if defect == 'stats_over_Tmax' else T_n
        xs = np.nan_to_num(x[n, :Ts]) if defect == 'stats_over_Tmax' else x[n, :Ts]
        if defect == 'tail_skip' and T_n > 7 * STAT_WAVES:
            xs = xs[:-1]
        cnt = Ts
        # a thread's chain over its ceil(T_n / 16) frames, the non-zero ones of the 16 partial sums, the division
        d_sum = -(-T_n // STAT_WAVES) + min(T_n, STAT_WAVES)
        M = Tr(xs.sum(axis=0) / cnt, np.abs(xs).sum(axis=0) / cnt, d_sum + 1)
        mean[n], meanb[n] = M.v, M.bound()
        xv = x[n, :T_n]
        D = Tr(xv) - Tr(np.broadcast_to(M.v, xv.shape), np.broadcast_to(M.a, xv.shape), M.d)      # cancellation: a = |x| + A_mean
        if T_n == 1:
            std[n] = np.nan
            out[n, :, :T_n] = np.nan
            continue
        # the squares are non-negative, their sum has no cancellation: (d + delta)^2 - d^2 = 2 d delta + delta^2 with delta the bound
        # of x - mean, then the square's rounding, the chain and the partial sums, the division, relative to the sum itself
        den = cnt if defect == 'biased' else cnt - 1
        dq = (xs - M.v) ** 2 if defect in ('tail_skip', 'stats_over_Tmax') else D.v ** 2
        delta = D.bound()
        var = dq.sum(axis=0) / den
        vb = (2 * np.abs(D.v) * delta + delta ** 2).sum(axis=0) / (T_n - 1) + (d_sum + 2 + 2) * U * var
        if defect == 'eps_under_root':
            s = np.sqrt(var + e)
        else:
            s = np.sqrt(var) + e
        # sqrt of a value known to vb: |sqrt(v') - sqrt(v)| <= vb / sqrt(v - vb) (sqrt(v + vb) if vb >= v); its own rounding and the add
        with np.errstate(divide='ignore', invalid='ignore'):
            sb = np.where(vb < var, vb / np.sqrt(np.maximum(var - vb, TINY)), np.sqrt(var + vb)) + 2 * LIBM_SQRTF * U * s + U * s
        std[n], stdb[n] = s, sb
        o = D.v / s
        with np.errstate(divide='ignore', invalid='ignore'):
            ob = D.bound() / s + np.abs(o) * np.where(sb < s, sb / (s - sb), np.inf) + U * np.abs(o) + TINY
        out[n, :, :T_n] = o.T
        outb[n, :, :T_n] = ob.T
    if defect == 'no_transpose_m64' and n_mels > 64:
        k = min(n_mels - 64, Tmax, 64)
        out[:, 64:64 + k, :k] = out[:, 64:64 + k, :k].transpose(0, 2, 1).copy()
    return out, outb, mean, meanb, std, stdb


# ---- log_softmax / softmax (ctc.hip log_softmax_fwd_kernel, log_softmax_bwd_kernel) ------------------------------------------------

def log_softmax_ref(logits, C, mode, defect=None):
    """logits [rows][CP] (columns >= C are junk) -> (out [rows][C], bound).  mode 0: log_softmax, 1: softmax.
    A row of -inf only gives NaN; -inf entries give -inf (mode 0) / 0 (mode 1) exactly."""
    x = np.asarray(logits, dtype=np.float64)
    xs = x[:, :C]
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        m = (x if defect == 'max_over_CP' else xs).max(axis=1, keepdims=True)
        dm = xs - m                                           # one rounding: u |x - m|
        ex = np.exp(dm)
        exb = ex * (U * np.where(np.isfinite(dm), np.abs(dm), 0.0) + 2 * LIBM_EXPF * U) + TINY * (ex > 0)
        if defect == 'skip_ge64':
            ex = ex.copy()
            ex[:, 64:] = 0.0
        s = ex.sum(axis=1, keepdims=True)
        d_s = -(-C // 64) + 6                                 # a lane's chain, the six shuffle levels
        sb = exb.sum(axis=1, keepdims=True) + (d_s + 2) * U * s
        ls = np.log(s)
        lsb = sb / s + 2 * LIBM_LOGF * U * np.abs(ls)
        lse = m + ls
        lseb = lsb + U * np.abs(lse)
        lp = xs - lse
        lpb = np.where(np.isfinite(lp), lseb + U * np.abs(lp), 0.0)
        if mode == 0:
            return lp, lpb
        p = np.exp(lp)
        pb = np.where(p > 0, p * (np.expm1(lpb) + 2 * LIBM_EXPF * U) + TINY, 0.0)
        return p, pb


def log_softmax_bwd_ref(gout, out, mode, defect=None):
    """mode 0: g - exp(out) * sum(g);  mode 1: out * (g - sum(g * out)).  gout, out [rows][C] (fp32 values) -> (glogits, bound)"""
    g = np.asarray(gout, dtype=np.float64)
    o = np.asarray(out, dtype=np.float64)
    C = g.shape[1]
    d_s = -(-C // 64) + 6
    with np.errstate(invalid='ignore', over='ignore'):
        if mode == 0:
            S = Tr(g.sum(axis=1, keepdims=True), np.abs(g).sum(axis=1, keepdims=True), d_s)
            E = Tr(np.exp(o), None, 2 * LIBM_EXPF)
            R = Tr(g) - E * S
        else:
            go = g * o
            if defect == 'bwd_sum_g':
                go = g
            S = Tr(go.sum(axis=1, keepdims=True), np.abs(go).sum(axis=1, keepdims=True), d_s + 1)
            R = Tr(o) * (Tr(g) - S)
        return R.v, R.bound() + TINY * (R.v != 0)


def argmax_ref(x):
    """the first NaN of a row, else the first maximum"""
    x = np.asarray(x)
    nan = np.isnan(x)
    return np.where(nan.any(axis=1), nan.argmax(axis=1), np.where(nan, -np.inf, x).argmax(axis=1)).astype(np.int32)


# ---- CTC (ctc_core.h ctc_alpha_beta_kernel, ctc_grad_kernel, ctc_loss_reduce_kernel, as w2l_ctc_loss of ctc.hip runs them) ---------

# one step  v = lse3(a0, a1, a2) + e  (lse3 = m + __logf(1 + __expf(md - m) + __expf(lo - m))):
#   each __expf: its argument's subtraction u |x| -> e^x u |x| <= u / e, and HW_EXPF_ABS u;  1 + e1 + e2 <= 3: two additions, 6u;
#   the logarithm's derivative is <= 1 on [1, 3], its own error HW_LOGF_ABS u;        -> K2
#   m + log(.) and . + e: one rounding each at magnitude <= max(|v|, |v - e|)         -> K1 = 2
K1 = 2.0
K2 = 2 * (HW_EXPF_ABS + 1 / math.e) + 6 + HW_LOGF_ABS
# gradient, relative to exp(lp) + post: expf(lp) 2 LIBM_EXPF; every expf term of acc 2 LIBM_EXPF and the n_c - 1 <= S additions of
# the states of one label; post_scale = expf(.) 2 LIBM_EXPF; acc * post_scale, the subtraction, * gs, and gs = 1 / (N * max(S, 1)):
# product and quotient, 2                                                            -> K3 = 6 LIBM_EXPF + S + 5
def k3(S):
    return 6 * LIBM_EXPF + S + 5


KWIDE = (64, 128, 192, 256, 320, 384, 448, 512, 640, 768, 896, 1024)


def ctc_variant(Smax, T, C):
    """(NT, SPT, LP_LDS) of the dispatch in w2l_ctc_loss"""
    L = 2 * Smax + 1
    assert L <= 8 * 1024
    nt = next((w for w in KWIDE if L <= w), 1024)
    spt = -(-L // nt)
    if spt > 1:
        spt = spt if spt <= 4 else (6 if spt <= 6 else 8)
    lds = 2 * (spt * nt + 4) * 4
    return nt, spt, lds + T * C * 4 <= 150 * 1024


def _lse(*xs):
    with np.errstate(invalid='ignore', divide='ignore'):
        m = functools.reduce(np.maximum, xs)
        ms = np.where(np.isfinite(m), m, 0.0)
        return np.where(np.isfinite(m), ms + np.log(sum(np.exp(x - ms) for x in xs)), -np.inf)


def _absmax(*xs):
    v = np.concatenate([np.ravel(x) for x in xs])
    v = v[np.isfinite(v)]
    return float(np.abs(v).max()) if v.size else 0.0


def _chain(em, skip, L, defect_nt=None):
    """alpha over rows 0.. of em [Tn][L] (the beta chain is the same on reversed arrays).  Returns (alpha [Tn][L], E [Tn])"""
    Tn = em.shape[0]
    al = np.full((Tn, L), -np.inf)
    al[0, :2] = em[0, :2]
    E = np.zeros(Tn)
    ninf1, ninf2 = np.full(1, -np.inf), np.full(2, -np.inf)
    if defect_nt is not None:
        al[0, defect_nt:] = -np.inf
    for t in range(1, Tn):
        a0 = al[t - 1]
        a1 = np.concatenate([ninf1, a0[:-1]])
        a2 = np.where(skip, np.concatenate([ninf2, a0[:-2]])[:L], -np.inf)
        lse = _lse(a0, a1, a2)
        with np.errstate(invalid='ignore'):
            al[t] = np.where(np.isfinite(lse), lse + em[t], -np.inf)
        if defect_nt is not None:
            al[t, defect_nt:] = -np.inf
        E[t] = E[t - 1] + U * (K1 * _absmax(al[t], lse) + K2)
    return al, E


def ctc_ref(lp, targets, in_len, tg_len, blank, zero_inf, Smax, want_grad=True, defect=None, nt=None):
    """lp [N][T][C] fp32 log-probabilities, targets [N][Smax].  Returns a dict: nll, nll_b [N]; loss, loss_b; grad, grad_b [N][T][C]
    (grad of an utterance with an infinite nll and zero_inf == 0 is NaN: not specified);  S, Tn: the clamped lengths."""
    lp = np.asarray(lp, dtype=np.float64)
    N, T, C = lp.shape
    nll = np.zeros(N)
    nllb = np.zeros(N)
    grad = np.zeros((N, T, C))
    gradb = np.zeros((N, T, C))
    Ss = np.clip(np.asarray(tg_len, dtype=np.int64), 0, Smax)
    Tns = np.clip(np.asarray(in_len, dtype=np.int64), 0, T)
    bl = 0 if defect == 'blank0' else blank
    for n in range(N):
        S, Tn = int(Ss[n]), int(Tns[n])
        L = 2 * S + 1
        gs = 1.0 / (N * (1 if defect == 'gs_noS' else max(S, 1)))
        if defect == 'rows_beyond':
            grad[n, Tn:] = np.exp(lp[n, Tn:]) * gs
        if Tn == 0:
            nll[n] = 0.0 if (S == 0 or zero_inf) else np.inf
            continue
        ext = np.full(L, bl, dtype=np.int64)
        ext[1::2] = targets[n, :S]
        s_idx = np.arange(L)
        odd = (s_idx & 1) == 1
        prev_lab = np.concatenate([[-1, -1], ext[:-2]])[:L]
        next_lab = np.concatenate([ext[2:], [-1, -1]])[:L]
        skip_a = odd & (s_idx >= 3) & ((prev_lab != ext) | (defect == 'skip_equal'))
        skip_b = odd & (s_idx + 2 < L) & ((next_lab != ext) | (defect == 'skip_equal'))
        if defect == 'no_skip3' and L > 3:
            skip_a[3] = False
        em = lp[n][:, ext]                                                    # [T][L]
        dnt = nt if defect == 'slot_ge_nt' else None
        al, Ea = _chain(em[:Tn], skip_a, L, dnt)
        a, b = al[Tn - 1, L - 1], (al[Tn - 1, L - 2] if L > 1 else -np.inf)
        v = -float(a if defect == 'lse2_last_only' else _lse(np.array(a), np.array(b)))
        Enll = Ea[Tn - 1] + U * (K1 * (abs(v) if np.isfinite(v) else 0.0) + K2)
        if not np.isfinite(v):
            if zero_inf:
                nll[n] = 0.0
            else:
                nll[n] = np.inf
                grad[n] = np.nan
            continue
        nll[n], nllb[n] = v, Enll
        if not want_grad:
            continue
        Tb = T if defect == 'beta_T' else Tn
        be_r, Eb_r = _chain(em[:Tb][::-1, ::-1], skip_b[::-1], L)          # the same chain on time- and state-reversed arrays
        be, Eb = be_r[::-1, ::-1][:Tn], Eb_r[::-1][:Tn]
        with np.errstate(invalid='ignore', over='ignore'):
            ab = al + be
            lpost = np.where(np.isfinite(ab), ab - em[:Tn] + v, -np.inf)
            post = np.zeros((Tn, C))
            contrib = np.exp(lpost)
            for c in np.unique(ext):
                post[:, c] = contrib[:, ext == c].sum(axis=1)
            elp = np.exp(lp[n, :Tn])
            # the roundings of al + be, - lp, - m and m + nll sit in the exponent at the magnitude of those sums
            Eloc = np.array([4 * U * (_absmax(ab[t]) + _absmax(lp[n, t]) + abs(v)) for t in range(Tn)])
            Etot = (Ea + Eb + Enll + Eloc)[:, None]
            grad[n, :Tn] = (elp - post) * gs
            gradb[n, :Tn] = gs * (post * np.expm1(Etot) + k3(S) * U * (elp + post)) + TINY
    terms = nll / np.maximum(Ss, 1)
    with np.errstate(invalid='ignore'):
        loss = terms.sum() / N
        # a thread's chain over ceil(N / 256) utterances, each a quotient; the 8-level tree; the division by N
        d = -(-N // 256) + 1 + 8 + 1
        loss_b = (nllb / np.maximum(Ss, 1)).sum() / N + (d + 2) * U * np.abs(terms[np.isfinite(terms)]).sum() / N
    return dict(nll=nll, nll_b=nllb, loss=loss, loss_b=loss_b, grad=grad, grad_b=gradb, S=Ss, Tn=Tns)


# ---- the cases the CPU and the GPU tests share ------------------------------------------------------------------------------------

PREEMPH, GUARD_LOG = 0.97, 2.0 ** -24


@dataclasses.dataclass(frozen=True)
class LogmelCase:
    n_fft: int
    win: int
    hop: int
    n_mels: int
    fb_range: bool
    dither: float          # 0: noise == NULL
    tmax_above: bool
    tone: bool

    @property
    def name(self):
        return (f'{self.n_fft}-{self.win}-{self.hop}-m{self.n_mels}-{"rng" if self.fb_range else "dense"}-d{self.dither:g}-'
                f'{"above" if self.tmax_above else "below"}-{"tone" if self.tone else "noise"}')


LOGMEL_CASES = [
    # the generic radix-2 kernel
    LogmelCase(64, 64, 32, 40, True, 0.0, True, False), LogmelCase(128, 100, 50, 64, False, 1e-5, False, True),
    LogmelCase(256, 256, 160, 80, True, 0.1, True, True), LogmelCase(1024, 800, 160, 128, False, 0.0, False, False),
    LogmelCase(256, 256, 160, 128, True, 1e-5, False, False), LogmelCase(1024, 800, 160, 40, True, 0.1, True, True),
    # the 8x8x8 kernel; hop >= 171: the samples are not staged in LDS
    LogmelCase(512, 320, 160, 40, True, 0.0, True, False), LogmelCase(512, 400, 160, 64, False, 1e-5, False, True),
    LogmelCase(512, 400, 170, 80, True, 0.1, True, False), LogmelCase(512, 400, 171, 128, False, 0.0, False, False),
    LogmelCase(512, 400, 200, 64, True, 1e-5, True, True), LogmelCase(512, 512, 256, 80, False, 0.1, False, False),
    LogmelCase(512, 400, 171, 40, True, 0.1, True, True),
]


@functools.lru_cache(maxsize=None)
def logmel_inputs(c):
    """three utterances: n_fft/2 + 1 samples, an exact multiple of hop, k*hop - 1; audio_stride above the longest"""
    rng = np.random.default_rng(1000 + LOGMEL_CASES.index(c))
    k = max(9, -(-5 * c.n_fft // (2 * c.hop)))
    ns = np.array([c.n_fft // 2 + 1, k * c.hop, (k + 1) * c.hop - 1], dtype=np.int32)
    stride = int(ns.max()) + 37
    i = np.arange(stride)
    if c.tone:
        audio = 0.5 * np.sin(2 * np.pi * 0.11 * i)[None, :] + 1e-4 * rng.standard_normal((3, stride))
    else:
        audio = 0.3 * rng.standard_normal((3, stride))
    audio = audio.astype(np.float32)
    noise = rng.standard_normal((3, stride)).astype(np.float32) if c.dither else None
    fbT, fr = filterbank(c.n_fft, c.n_mels)
    frames = int(1 + ns.max() // c.hop)
    Tmax = frames + 3 if c.tmax_above else frames - 2
    return dict(audio=audio, ns=ns, stride=stride, noise=noise, window=hann(c.win), fbT=fbT, fb_range=fr if c.fb_range else None,
                Tmax=Tmax)


def logmel_case_ref(c, defect=None):
    D = logmel_inputs(c)
    return logmel_ref(D['audio'], D['ns'], D['noise'], c.dither, PREEMPH, D['window'], c.n_fft, c.hop, D['fbT'], D['fb_range'],
                      GUARD_LOG, D['Tmax'], defect)


NORM_HOP, NORM_EPS = 160, 1e-5
NORM_TN = (1, 2, 16, 17, 112, 113, 128, 129, 300, 330)          # the last: more frames than Tmax
NORM_CASES = [(40, 300), (64, 320), (80, 300), (128, 320)]      # (n_mels, Tmax)


@functools.lru_cache(maxsize=None)
def normalize_inputs(n_mels, Tmax):
    rng = np.random.default_rng(2000 + n_mels)
    ns = np.array([(t - 1) * NORM_HOP + (7 * i) % NORM_HOP for i, t in enumerate(NORM_TN)], dtype=np.int32)
    x = np.abs(3.0 + rng.standard_normal((len(ns), Tmax, n_mels))).astype(np.float32)
    two = NORM_TN.index(2)                                       # two frames: kept apart, or the variance is all cancellation
    x[two, 1] = x[two, 0] + rng.choice([-1.0, 1.0], size=n_mels) * (0.5 + rng.random(n_mels))
    for n, t in enumerate(NORM_TN):
        x[n, min(t, Tmax):] = np.nan                             # never read
    return x, ns


SOFTMAX_SHAPES = [(3, 50, 29, 64), (1, 7, 29, 29), (2, 5, 1, 64), (1, 3, 64, 64), (2, 9, 65, 128), (1, 6, 200, 256)]


@functools.lru_cache(maxsize=None)
def softmax_inputs(shape):
    """rows cycle through: scale 3; near +-1e4; some -inf; (from the fourth row on) all -inf.  Columns C..CP hold NaN."""
    N, T, C, CP = shape
    rng = np.random.default_rng(3000 + C + CP)
    rows = N * T
    x = np.full((rows, CP), np.nan, dtype=np.float32)
    for r in range(rows):
        kind = r % 4
        v = 3.0 * rng.standard_normal(C)
        if kind == 1:
            v = v + 1e4 * rng.choice([-1.0, 1.0], size=C)
        elif kind == 2:
            v[1:][rng.random(C - 1) < 0.3] = -np.inf
        elif kind == 3:
            v[:] = -np.inf
        x[r, :C] = v
    gout = rng.standard_normal((rows, C)).astype(np.float32)
    return x, gout


@dataclasses.dataclass
class CtcCase:
    name: str
    kind: str                  # 'tight', 'full', 'sem'
    lp: np.ndarray
    targets: np.ndarray
    in_len: np.ndarray
    tg_len: np.ndarray
    Smax: int
    blank: int = 0
    zero_inf: int = 1
    want_grad: bool = True
    torch_ok: bool = True      # lengths torch accepts as they are
    infinite: bool = False     # built for infinities

    @property
    def dims(self):
        return self.lp.shape

    @property
    def variant(self):
        N, T, C = self.lp.shape
        return ctc_variant(self.Smax, T, C)


def _log_probs(rng, N, T, C, scale=1.0):
    x = scale * rng.standard_normal((N, T, C))
    x = x - x.max(axis=2, keepdims=True)
    return (x - np.log(np.exp(x).sum(axis=2, keepdims=True))).astype(np.float32)


def _targets(rng, N, Smax, lens, C, blank, repeats=True):
    tg = np.zeros((N, max(Smax, 1)), dtype=np.int32)
    labels = np.array([c for c in range(C) if c != blank])
    for n in range(N):
        t = rng.choice(labels, size=int(lens[n]))
        if not repeats:
            for i in range(1, len(t)):
                if t[i] == t[i - 1]:
                    t[i] = labels[(np.where(labels == t[i])[0][0] + 1) % len(labels)]
        tg[n, :len(t)] = t
    return tg


# Smax at both edges of every kWide / spt range -> the 17 (NT, SPT) pairs
TIGHT_SMAX = [31, 32, 63, 64, 95, 96, 127, 128, 159, 160, 191, 192, 223, 224, 255, 256, 319, 320, 383, 384, 447, 448, 511,
              512, 1023, 1024, 1535, 1536, 2047, 2048, 3071, 3072, 4095]
TIGHT_TN = 40


@functools.lru_cache(maxsize=None)
def ctc_tight_case(Smax, staged):
    """Smax sizes the buffers and picks the kernel; the live problem is small (S <= 6 of few labels, 40 frames) so that the
    bound stays tight.  staged: C = 29, T = 48; not staged: C = 64, T = 600 (T*C*4 = 153 600 > 150 KB - the recursion's buffers)."""
    rng = np.random.default_rng(4000 + Smax * 2 + staged)
    N = 2
    T, C = (48, 29) if staged else (600, 64)
    lp = _log_probs(rng, N, T, C, 0.5)
    lens = np.array([6, 3], dtype=np.int32)
    tg = _targets(rng, N, Smax, lens, C, 0)
    tg[:, 6:] = -7                                                # padding: never a valid label, never read
    c = CtcCase(f'tight-S{Smax}-{"lds" if staged else "mem"}', 'tight', lp, tg, np.array([TIGHT_TN, TIGHT_TN - 7], dtype=np.int32),
                lens, Smax)
    assert c.variant[2] == bool(staged)
    return c


def ctc_tight_cases():
    seen, out = set(), []
    for staged in (1, 0):
        for Smax in TIGHT_SMAX:
            v = ctc_variant(Smax, 48 if staged else 600, 29 if staged else 64)
            if staged or v not in seen:                           # both edges staged, one edge from memory
                seen.add(v)
                out.append((Smax, staged))
    return out


FULL_SMAX = [511, 1023, 1535, 2047, 3071, 4095]                  # 1024 x 1, and SPT = 2, 3, 4, 6, 8


@functools.lru_cache(maxsize=None)
def ctc_full_case(Smax):
    """target lengths close to Smax: states in every slot of a thread are live"""
    rng = np.random.default_rng(5000 + Smax)
    C = 29
    S = Smax - 3
    tg = _targets(rng, 1, Smax, [S], C, 0)
    rep = int((tg[0, 1:S] == tg[0, :S - 1]).sum())
    T = S + rep + 40
    lp = _log_probs(rng, 1, T, C, 1.0)
    return CtcCase(f'full-S{Smax}', 'full', lp, tg, np.array([T], dtype=np.int32), np.array([S], dtype=np.int32), Smax)


def _one_path(rng, S, T, C, zero_inf, name):
    """utterance 0: one label S times in T frames (T == 2S - 1: exactly one path; 2S - 2: none); utterance 1: ordinary"""
    lp = _log_probs(rng, 2, T, C)
    tg = np.zeros((2, S), dtype=np.int32)
    tg[0] = 5
    tg[1] = _targets(rng, 1, S, [S], C, 0, repeats=False)[0]
    tl = np.array([S, min(S, T // 2)], dtype=np.int32)
    return CtcCase(name, 'sem', lp, tg, np.array([T, T], dtype=np.int32), tl, S, 0, zero_inf, infinite=T < 2 * S - 1)


@functools.lru_cache(maxsize=None)
def ctc_sem_cases():
    out = []
    rng = np.random.default_rng(6000)
    for C in (2, 29, 64):
        for blank in sorted({0, 13 % C, C - 1}):
            N, T, Smax = 3, 24, 7
            lens = np.array([7, 4, 1], dtype=np.int32)
            out.append(CtcCase(f'blank{blank}-C{C}', 'sem', _log_probs(rng, N, T, C), _targets(rng, N, Smax, lens, C, blank),
                               np.array([T, T - 5, T - 11], dtype=np.int32), lens, Smax, blank))
    # repeated labels throughout
    lens = np.array([8, 6], dtype=np.int32)
    tg = np.array([[3, 3, 3, 4, 4, 3, 3, 9], [7, 7, 7, 7, 7, 7, 0, 0]], dtype=np.int32)
    tg[tg == 0] = 1
    out.append(CtcCase('repeats', 'sem', _log_probs(rng, 2, 30, 29), tg, np.array([30, 22], dtype=np.int32), lens, 8))
    out.append(_one_path(rng, 9, 17, 29, 1, 'one-path'))
    out.append(_one_path(rng, 9, 16, 29, 1, 'no-path-zero-inf'))
    out.append(_one_path(rng, 9, 16, 29, 0, 'no-path-inf'))
    # S == 0; input_lengths == 0 with S == 0 and S > 0; input_lengths < T
    lens = np.array([0, 0, 4, 5], dtype=np.int32)
    for zi in (1, 0):
        out.append(CtcCase(f'empty-zi{zi}', 'sem', _log_probs(rng, 4, 20, 29), _targets(rng, 4, 6, lens, 29, 0),
                           np.array([20, 0, 0, 13], dtype=np.int32), lens, 6, 0, zi, torch_ok=False, infinite=zi == 0))
    # lengths outside their ranges: clamped
    out.append(CtcCase('clamped', 'sem', _log_probs(rng, 4, 20, 29), _targets(rng, 4, 5, [5, 5, 5, 5], 29, 0),
                       np.array([25, 20, 1000, 12], dtype=np.int32), np.array([9, -3, 5, 100], dtype=np.int32), 5, torch_ok=False))
    # grad == NULL
    lens = np.array([5, 2], dtype=np.int32)
    out.append(CtcCase('no-grad', 'sem', _log_probs(rng, 2, 20, 29), _targets(rng, 2, 5, lens, 29, 0),
                       np.array([20, 15], dtype=np.int32), lens, 5, want_grad=False))
    # -inf log-probabilities: every label outside the target, and one target label in one frame
    lens = np.array([4, 3], dtype=np.int32)
    tg = _targets(rng, 2, 4, lens, 29, 0, repeats=False)
    lp = _log_probs(rng, 2, 20, 29)
    for n in range(2):
        outside = np.setdiff1d(np.arange(1, 29), tg[n, :lens[n]])
        lp[n][:, outside] = -np.inf
    lp[0, 9, tg[0, 1]] = -np.inf
    out.append(CtcCase('neg-inf-lp', 'sem', lp, tg, np.array([20, 20], dtype=np.int32), lens, 4))
    # N > 256: the loop of the loss reduction
    N = 257
    lens = rng.integers(0, 4, size=N).astype(np.int32)
    out.append(CtcCase('N257', 'sem', _log_probs(rng, N, 8, 29), _targets(rng, N, 3, lens, 29, 0, repeats=False),
                       rng.integers(7, 9, size=N).astype(np.int32), lens, 3))
    return out


_REF_CACHE = {}


def ctc_case_ref(c, defect=None, want_grad=True):
    """the reference of a shared case, computed once (a defective one is not kept)"""
    key = (c.name, defect)
    if key not in _REF_CACHE:
        r = ctc_ref(c.lp, c.targets, c.in_len, c.tg_len, c.blank, c.zero_inf, c.Smax, c.want_grad and want_grad, defect,
                    nt=c.variant[0])
        if defect is not None:
            return r
        _REF_CACHE[key] = r
    return _REF_CACHE[key]
