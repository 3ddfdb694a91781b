"""Float64 reference of the wildcard CTC loss (csrc/wctc.hip, w2l_wctc_loss): ctc_ref of frontend_refs.py restated for the
definition in include/w2l_hip.h -- plain NumPy, nothing of the package's Python.  It returns the exact values AND per-element
bounds of what the fp32 device kernels may differ by.

The bound is ctc_ref's, with omega treated as one more emitting class:
  * the recursion is the same chain (frontend_refs._chain: K1, K2 per step).  A wildcard gap's emission is the constant
    ``penalty``, an exact fp32 number, where a plain gap's is an exact fp32 log-probability: the step  v = lse3(.) + e  has the same
    roundings, so alpha, beta and nll carry the same accumulated bounds Ea, Eb, Enll;
  * a state posterior is exp(al + be - e + nll): the roundings of al + be, - e, - m and m + nll sit in the exponent at the
    magnitude of those sums (Eloc; |penalty| is counted like the frame's log-probabilities).  So every linear-domain sum of state
    posteriors -- post(t,c) of a class, and omega(t) of the wildcard gaps alike -- is off by the factor expm1(Etot) from the
    exponent, and by ctc_ref's relative roundings: each expf term 2 LIBM_EXPF, the n - 1 <= S additions of the states of one
    slot (the wildcard slot holds at most S + 1 gaps: S additions), post_scale 2 LIBM_EXPF, the product;
  * grad = ((expf(lp) - post) - expf(lp) * omega) * gs, the kernel's order of exp(lp) (1 - omega) - post: beyond ctc_ref's count
    k3(S) (which already holds expf(lp), the first subtraction, * gs and gs itself) come the product expf(lp) * omega and its
    subtraction: two more roundings, relative to expf(lp) (1 + omega) + post.  omega's own error enters scaled by expf(lp).
  ->  grad_b = gs * ((post + elp * omega) * expm1(Etot) + (k3(S) + 2) u (elp * (1 + omega) + post)) + TINY.
With omega == 0 this is ctc_ref's bound with k3 + 2 in place of k3.

``defect=``: a named, deliberate fault that models a kernel bug (test_cpu_wctc.py shows that each one leaves the bound on a case
the GPU tests run)."""
import dataclasses
import functools

import numpy as np

from frontend_refs import K1, K2, TINY, _absmax, _chain, _log_probs, _lse, ctc_variant, k3
from kernel_refs import U

DEFECTS = ['wild_as_blank', 'omega_dropped', 'flag_shifted', 'trailing_flag_lost', 'stars_counted_in_S', 'stars_not_merged',
           'penalty_ignored']


def parse_row(row, R, star, C, blank, defect=None):
    """raw row -> (labels z [S], gap flags w [S + 1], bad): the parsing rule of the definition"""
    z, gaps, bad = [], [], False
    run = 0
    for v in list(row[:R]):
        v = int(v)
        if v == star:
            # merged: every star of a run flags the gap it stands in; the defect lets the q-th star of a run spill q gaps on
            gaps.append(len(z) + (run if defect == 'stars_not_merged' else 0))
            run += 1
            continue
        run = 0
        if v < 0 or v >= C or v == blank:
            bad = True
        z.append(v)
    S = len(z)
    w = np.zeros(S + 1, dtype=bool)
    for g in gaps:
        w[min(g, S)] = True
    if defect == 'flag_shifted':
        w = np.concatenate([[False], w[:-1]])
    if defect == 'trailing_flag_lost':
        w[S] = False
    return np.array(z, dtype=np.int64), w, bad


def wctc_ref(lp, targets, in_len, tg_len, blank, zero_inf, Smax, star, penalty, want_grad=True, defect=None):
    """lp [N][T][C] fp32 log-probabilities, targets [N][Smax] raw rows (labels and ``star``), tg_len the raw lengths.  Returns a
    dict: nll, nll_b [N]; loss, loss_b; grad, grad_b [N][T][C] (grad of an utterance with an infinite nll and zero_inf == 0 is
    NaN: not specified); status [N]; S (labels per row), Tn (clamped input lengths)."""
    lp = np.asarray(lp, dtype=np.float64)
    N, T, C = lp.shape
    nll, nllb = np.zeros(N), np.zeros(N)
    grad, gradb = np.zeros((N, T, C)), np.zeros((N, T, C))
    status = np.zeros(N, dtype=np.int32)
    Rs = np.clip(np.asarray(tg_len, dtype=np.int64), 0, Smax)
    Tns = np.clip(np.asarray(in_len, dtype=np.int64), 0, T)
    Ss = np.zeros(N, dtype=np.int64)
    pen = 0.0 if defect == 'penalty_ignored' else float(np.float32(penalty))
    for n in range(N):
        R, Tn = int(Rs[n]), int(Tns[n])
        z, w, bad = parse_row(targets[n] if Smax else [], R, star, C, blank, defect)
        S = len(z)
        Ss[n] = S + int((np.asarray(targets[n][:R]) == star).sum()) if defect == 'stars_counted_in_S' else S
        if bad:
            status[n] = 2                                                     # nll, loss term and gradient 0
            continue
        L = 2 * S + 1
        gs = 1.0 / (N * max(int(Ss[n]), 1))
        if Tn == 0:
            if S > 0:
                status[n] = 1
                nll[n] = 0.0 if zero_inf else np.inf
            continue
        ext = np.full(L, blank, dtype=np.int64)
        ext[1::2] = z
        wild = np.zeros(L, dtype=bool)
        if defect != 'wild_as_blank':
            wild[0::2] = w
        s_idx = np.arange(L)
        odd = (s_idx & 1) == 1
        prev_lab = np.concatenate([[-1, -1], ext[:-2]])[:L]
        next_lab = np.concatenate([ext[2:], [-1, -1]])[:L]
        skip_a = odd & (s_idx >= 3) & (prev_lab != ext)
        skip_b = odd & (s_idx + 2 < L) & (next_lab != ext)
        em = np.where(wild[None, :], pen, lp[n][:, ext])                      # [T][L]
        al, Ea = _chain(em[:Tn], skip_a, L)
        a, b = al[Tn - 1, L - 1], (al[Tn - 1, L - 2] if L > 1 else -np.inf)
        v = -float(_lse(np.array(a), np.array(b)))
        Enll = Ea[Tn - 1] + U * (K1 * (abs(v) if np.isfinite(v) else 0.0) + K2)
        if not np.isfinite(v):
            status[n] = 1
            if zero_inf:
                nll[n] = 0.0
            else:
                nll[n] = np.inf
                grad[n] = np.nan
            continue
        nll[n], nllb[n] = v, Enll
        if not want_grad:
            continue
        be_r, Eb_r = _chain(em[:Tn][::-1, ::-1], skip_b[::-1], L)          # the same chain on time- and state-reversed arrays
        be, Eb = be_r[::-1, ::-1], Eb_r[::-1]
        with np.errstate(invalid='ignore', over='ignore'):
            ab = al + be
            gamma = np.exp(np.where(np.isfinite(ab), ab - em[:Tn] + v, -np.inf))   # state posteriors: each frame's sum to 1
            post = np.zeros((Tn, C))
            for c in np.unique(ext):
                post[:, c] = gamma[:, (ext == c) & ~wild].sum(axis=1)
            omega = gamma[:, wild].sum(axis=1)[:, None]
            if defect == 'omega_dropped':
                omega = np.zeros_like(omega)
            elp = np.exp(lp[n, :Tn])
            Eloc = np.array([4 * U * (_absmax(ab[t]) + max(_absmax(lp[n, t]), abs(pen)) + abs(v)) for t in range(Tn)])
            Etot = (Ea + Eb + Enll + Eloc)[:, None]
            grad[n, :Tn] = (elp * (1.0 - omega) - post) * gs
            gradb[n, :Tn] = gs * ((post + elp * omega) * np.expm1(Etot) + (k3(S) + 2) * U * (elp * (1.0 + omega) + post)) + TINY
    terms = nll / np.maximum(Ss, 1)
    with np.errstate(invalid='ignore'):
        loss = terms.sum() / N
        # a thread's chain over ceil(N / 256) utterances, each a quotient; the 8-level tree; the division by N (as ctc_ref)
        d = -(-N // 256) + 1 + 8 + 1
        loss_b = (nllb / np.maximum(Ss, 1)).sum() / N + (d + 2) * U * np.abs(terms[np.isfinite(terms)]).sum() / N
    return dict(nll=nll, nll_b=nllb, loss=loss, loss_b=loss_b, grad=grad, grad_b=gradb, status=status, S=Ss, Tn=Tns)


# ---- the cases the CPU and the GPU tests share ------------------------------------------------------------------------------------

C_CASE, N_CASE, BLANK = 29, 3, 0
STAR = C_CASE

# (name, Smax, T): the edges of w2l_wctc_loss's dispatch -- L = 2 Smax + 1 <= 64; L = 65 and 129 (the next two widths); L just
# above 1024 (two states per thread); log-probabilities too large for LDS (T * C * 4 > 150 KB) with a small Smax
SHAPES = [('L63', 31, 56), ('L65', 32, 80), ('L129', 64, 160), ('L1025', 512, 600), ('mem', 8, 1400)]
PATTERN_GROUPS = [('none', 'leading', 'trailing'), ('both', 'every_gap', 'equal_labels'), ('consecutive', 'star_only', 'empty')]
PENALTIES = (0.0, -0.5)


def _labels(rng, S, repeats=True):
    t = rng.integers(1, C_CASE, size=S)
    if not repeats:
        for i in range(1, S):
            if t[i] == t[i - 1]:
                t[i] = t[i] % (C_CASE - 1) + 1
    return [int(v) for v in t]


def pattern_row(rng, name, R):
    """a raw row of at most R entries in the named flag pattern"""
    if name == 'none':
        return _labels(rng, R)
    if name == 'leading':
        return [STAR] + _labels(rng, R - 1)
    if name == 'trailing':
        return _labels(rng, R - 1) + [STAR]
    if name == 'both':
        return [STAR] + _labels(rng, R - 2) + [STAR]
    if name == 'every_gap':
        row = [STAR]
        for v in _labels(rng, (R - 1) // 2):
            row += [v, STAR]
        return row
    if name == 'equal_labels':                                # a star between equal labels (every third gap), plain repeats too
        z = _labels(rng, (3 * R) // 4)
        row = []
        for i, v in enumerate(z):
            if i and i % 3 == 0:
                row += [STAR, z[i - 1]]
            else:
                row.append(v)
        return row[:R] if row[R - 1:R] != [STAR] else row[:R - 1]
    if name == 'consecutive':                                 # runs of two and three stars: at the start, inside, at the end
        z = _labels(rng, max((R - 5) // 2, 1))
        row = [STAR, STAR]
        for i, v in enumerate(z):
            row.append(v)
            if i % 4 == 1 and i + 1 < len(z):
                row += [STAR] * (2 + (i // 4) % 2)
        return (row + [STAR, STAR, STAR])[:R]
    if name == 'star_only':
        return [STAR] * R
    assert name == 'empty'
    return []


@dataclasses.dataclass(frozen=True, eq=False)
class WctcCase:
    name: str
    lp: np.ndarray
    targets: np.ndarray
    in_len: np.ndarray
    tg_len: np.ndarray
    Smax: int
    penalty: float = 0.0
    zero_inf: int = 1
    want_grad: bool = True

    @property
    def dims(self):
        return self.lp.shape

    @property
    def variant(self):
        N, T, C = self.lp.shape
        return ctc_variant(self.Smax, T, C)


def _rows_case(name, rng, rows, Smax, T, in_len, penalty, zero_inf=1, scale=1.0):
    tg = np.full((len(rows), max(Smax, 1)), -7, dtype=np.int32)        # padding: never a valid entry, never read
    for n, r in enumerate(rows):
        assert len(r) <= Smax
        tg[n, :len(r)] = r
    return WctcCase(name, _log_probs(rng, len(rows), T, C_CASE, scale), tg, np.asarray(in_len, dtype=np.int32),
                    np.array([len(r) for r in rows], dtype=np.int32), Smax, penalty, zero_inf)


@functools.lru_cache(maxsize=None)
def shape_case(shape, group, penalty):
    """N = 3 rows, one flag pattern each, as long as the row width allows; input lengths T, T - 7 and T - 13 (shape 'mem': T, 40
    and 33, so that two rows keep a tight bound under the 1400-frame buffer)"""
    name, Smax, T = SHAPES[shape]
    rng = np.random.default_rng(7000 + 100 * shape + 10 * group + (penalty != 0.0))
    rows = [pattern_row(rng, pat, Smax) for pat in PATTERN_GROUPS[group]]
    in_len = [T, 40, 33] if name == 'mem' else [T, T - 7, T - 13]
    return _rows_case(f'{name}-{"+".join(PATTERN_GROUPS[group])}-p{penalty:g}', rng, rows, Smax, T, in_len, penalty)


def shape_cases():
    return [(s, g, p) for s in range(len(SHAPES)) for g in range(len(PATTERN_GROUPS)) for p in PENALTIES]


@functools.lru_cache(maxsize=None)
def star_free_case(shape):
    """rows without a star: what w2l_ctc_loss computes too"""
    name, Smax, T = SHAPES[shape]
    rng = np.random.default_rng(7900 + shape)
    rows = [_labels(rng, Smax), _labels(rng, max(Smax // 2, 1)), _labels(rng, min(Smax, 3))]
    in_len = [T, 40, 33] if name == 'mem' else [T, T - 7, T - 13]
    return _rows_case(f'{name}-star-free', rng, rows, Smax, T, in_len, 0.0)


@functools.lru_cache(maxsize=None)
def bad_entry_case():
    """row 1 holds the blank, row 2 an id past the star, row 3 a negative one: status 2, loss and gradient 0; rows 0 and 4 are fine"""
    rng = np.random.default_rng(7950)
    rows = [[STAR, 3, 4, STAR, 5], [3, BLANK, 4], [3, STAR + 1, 4, STAR], [-1, 3], [7, 7, STAR, 7]]
    return _rows_case('bad-entry', rng, rows, 6, 24, [24, 24, 20, 24, 17], -0.5)


@functools.lru_cache(maxsize=None)
def infeasible_case(zero_inf):
    """row 0: one label nine times in 16 frames with plain gaps (17 are needed): no path; row 1: the same labels with a star in
    every gap -- a wildcard gap still needs its frame between equal labels: no path either; row 2: 17 frames' worth, feasible"""
    rng = np.random.default_rng(7960)
    rows = [[5] * 9, [5, STAR] * 9, [5, STAR] * 8 + [5], [STAR, 6, 7]]
    c = _rows_case(f'infeasible-zi{zero_inf}', rng, rows, 18, 17, [16, 16, 17, 0], 0.0, zero_inf)
    return c


_REF_CACHE = {}


def case_ref(c, defect=None, want_grad=True):
    """the reference of a shared case, computed once (a defective one is not kept)"""
    if defect is not None or not want_grad:
        return wctc_ref(c.lp, c.targets, c.in_len, c.tg_len, BLANK, c.zero_inf, c.Smax, STAR, c.penalty, want_grad, defect)
    if c.name not in _REF_CACHE:
        _REF_CACHE[c.name] = wctc_ref(c.lp, c.targets, c.in_len, c.tg_len, BLANK, c.zero_inf, c.Smax, STAR, c.penalty)
    return _REF_CACHE[c.name]
