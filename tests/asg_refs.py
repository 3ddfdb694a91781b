"""Float64 references of the ASG criterion and its Viterbi decoder (torch on the CPU, NumPy), written from the definitions:

  Z_full = logsumexp over all A^T frame paths of  sum_t x[t, pi_t] + sum_{t>=1} g[pi_{t-1}, pi_t]
  Z_tgt  = the same over the paths that read the encoded target y, every label held for at least one frame
  loss   = Z_full - Z_tgt

``full_logz`` / ``target_logz`` are the two recursions as plain torch.logsumexp loops (autograd gives the gradients);
``brute_force`` enumerates every path and pins those recursions; ``viterbi`` is the best path with ties to the lowest
predecessor and the lowest final label.

``asg_ref`` is the definition of include/w2l_hip.h once more, in plain NumPy float64 with the intermediate tables kept, because the
per-element bounds of what the fp32 kernels of csrc/asg.hip may differ by need them (test_cpu_asg.py pins it to ``asg_loss`` and
``brute_force``).  The bounds follow the kernels' arithmetic with the rules of kernel_refs.py / frontend_refs.py (u = 2^-24, a
result reached through d roundings obeys |got - ref| <= (d + 2) u A; a k-ulp function counts as 2k roundings):

  full chain, one frame   v_j = e_j + ms_j + __logf(sum_k __expf(c_kj - ms_j)),  c_kj = cur_k + g_kj,  ms_j = max_k c_kj.
      c_kj: one rounding, u |c_kj|, beside the error E[t-1][k] the previous frame handed on: d_kj in all.  Through the log-sum-exp
      they pass weighted: by the mean value theorem its change is sum_k p_k(xi) d_k with the softmax weights p at a point xi of the
      segment, where no argument has moved by more than dmax = max_k d_k, so p_k(xi) <= min(1, p_k e^(2 dmax)); and it is at most dmax
      (1-Lipschitz).   -> min(dmax, sum_k min(1, p_kj e^(2 dmax)) d_kj), one bound per label and frame (a label far below the others has
      a large |c| and rounds coarsely, but weighs nothing).  The maximum is exact.  Each __expf of an argument <= 0 is off by
      u (HW_EXPF_ABS + 1/e) absolutely (the subtraction's rounding u |x| e^x <= u / e); the padding lanes hold -inf, their terms are
      exactly 0 and adding 0 is exact, so A terms and A - 1 additions of partial sums <= s count, not AP.  s >= 1 (the maximum's own
      term is exp(0)), so the logarithm's derivative is <= 1; __logf itself (2 HW_LOG + 2) u ln s <= (2 HW_LOG + 2) u ln max(A, 3).
        -> K2_full(A) = A (HW_EXPF_ABS + 1/e) + (A - 1) + (2 HW_LOG + 2) ln max(A, 3)
      e + ms and . + log s: one rounding each                                   -> K1_full = 1 at each of |c|, |e + ms|, |v|
      E[t][j] = min(dmax, sum_k min(1, p_kj e^(2 dmax)) d_kj) + u (|e_j + ms_j| + |v_j| + K2_full), accumulated frame by frame as
      frontend_refs._chain accumulates its E[t], but per label.
  zf   m + logf(sum_k expf(cur_k - m)) over a 64-lane butterfly (6 additions deep), libm:  E[Tn-1] through the log-sum-exp as above,
      + u (A / e + 2 LIBM_EXPF + 6 + 2 LIBM_LOGF ln s + |zf| + 2).
  target chain, one frame   v = lse2(cur + g_stay, prev + g_adv) + e: CTC's step with two terms.  The two sums, m + log and . + e:
      one rounding each at |a|, |b| (weighted through the lse2 like the full chain's, per state), |lse|, |v|; two __expf (one of
      them exp(0)), one addition of a sum <= 2, __logf on [1, 2]
        -> K2_tgt = 2 (HW_EXPF_ABS + 1/e) + 2 + HW_LOGF_ABS.
      Only the states a path can be in at frame t (max(0, S - (Tn - t)) <= s <= min(S - 1, t)) count: a state outside feeds no
      state inside, and its posterior is 0 through the -inf of the other chain.  zt = alpha[Tn-1][S-1] carries that chain's bound.
  nll = zf - zt: the two bounds and one rounding.  loss: a quotient per utterance ('mean'), N additions in order, the division by N.
  posteriors   every rounding of an exponent enters as expm1(Etot):  P_full(t, i) = expf(fa + fb - x - zf): Efa[t] + Efb[t] + Ezf,
      the three roundings of the sums at their magnitudes, expf 2 LIBM_EXPF (+ 2).  State posteriors expf(ta + tb - x - zt) and the
      pair posteriors expf(fa[t-1,i] + g_ij + fb[t,j] - zf), expf(ta[t-1,s'] + g + tb[t,s] - zt) likewise.
  linear-domain sums carry their additions relative to the sum (all terms >= 0): the n_i states of one label at a frame n_i - 1;
      a slab entry at most TCH - 1 = 63 frame additions, then the n_ij matching states of ``sub``; the N * chunks slabs in order.
  differences   (P_full - P_tgt) * w_n: the subtraction, the product, and w_n = 1 / (N * S) (a product and a quotient), + 2: 6 u
      relative to P_full + P_tgt, NOT to their difference.  A result flushed to zero: TINY.
  Rows t >= Tn, infeasible (status 1) and bad (status 2) utterances are exact zeros: bound 0.

``defect=``: a named, deliberate fault that models a kernel bug (test_cpu_asg.py shows that each one leaves the bound on a case of
the table below, which the GPU tests run)."""
import dataclasses
import functools
import itertools
import math

import numpy as np
import torch

from frontend_refs import HW_EXPF_ABS, HW_LOG, HW_LOGF_ABS, LIBM_EXPF, LIBM_LOGF, TINY, _lse
from kernel_refs import U


def encode(labels, repeat=0):
    """the repetition encoding, written independently of the package's: 2nd, 4th, ... member of a run -> repeat"""
    out = []
    i = 0
    labels = [int(v) for v in labels]
    while i < len(labels):
        j = i
        while j < len(labels) and labels[j] == labels[i]:
            out.append(repeat if (j - i) % 2 else labels[i])
            j += 1
        i = j
    return out


def full_logz(x, g):
    """x [T, A], g [A, A] (float64 tensors) -> Z_full"""
    alpha = x[0]
    for t in range(1, x.shape[0]):
        alpha = x[t] + torch.logsumexp(alpha[:, None] + g, dim=0)
    return torch.logsumexp(alpha, dim=0)


def target_logz(x, g, y):
    """x [T, A], g [A, A], y: encoded target (no two neighbours equal), 1 <= len(y) <= T -> Z_tgt"""
    y = torch.as_tensor(y, dtype=torch.long)
    S = len(y)
    # "impossible" is -1e30, not -inf: exp(-1e30 - m) is exactly 0 in float64 just the same, and the gradient of a
    # logsumexp over two impossible entries stays 0 instead of becoming 0 / 0
    neg = torch.full((1,), -1e30, dtype=x.dtype)
    stay = g[y, y]
    adv = g[y[:-1], y[1:]]
    alpha = torch.cat([x[0, y[:1]], neg.expand(S - 1)])
    for t in range(1, x.shape[0]):
        moved = torch.cat([neg, alpha[:-1] + adv])
        alpha = x[t, y] + torch.logsumexp(torch.stack([alpha + stay, moved]), dim=0)
    return alpha[S - 1]


def asg_loss(x, g, targets, in_lens, repeat=0, reduction='mean'):
    """batch reference.  x [N, T, A] and g [A, A] array-likes, targets: RAW transcripts (lists of ints), in_lens [N].
    -> dict(loss, nll [N], grad_x [N, T, A], grad_g [A, A]) in float64; infeasible utterances (S = 0 or S > T_n) give 0."""
    x = torch.as_tensor(np.asarray(x), dtype=torch.float64).clone().requires_grad_(True)
    g = torch.as_tensor(np.asarray(g), dtype=torch.float64).clone().requires_grad_(True)
    N = x.shape[0]
    nll, terms = [], []
    for n in range(N):
        y = encode(targets[n], repeat)
        Tn = int(in_lens[n])
        if len(y) == 0 or len(y) > Tn:
            nll.append(torch.zeros((), dtype=torch.float64))
        else:
            xn = x[n, :Tn]
            nll.append(full_logz(xn, g) - target_logz(xn, g, y))
        terms.append(nll[-1] / max(len(y), 1) if reduction == 'mean' else nll[-1])
    loss = sum(terms) / N if reduction == 'mean' else sum(terms)
    if loss.requires_grad:
        loss.backward()
    gx = x.grad if x.grad is not None else torch.zeros_like(x)
    gg = g.grad if g.grad is not None else torch.zeros_like(g)
    return dict(loss=float(loss.detach()), nll=np.array([float(v.detach()) for v in nll]), grad_x=gx.numpy().copy(), grad_g=gg.numpy().copy())


def collapse(path):
    out = []
    for v in path:
        if not out or out[-1] != v:
            out.append(int(v))
    return out


def path_score(x, g, path):
    s = x[0, path[0]]
    for t in range(1, len(path)):
        s = s + g[path[t - 1], path[t]] + x[t, path[t]]
    return s


def brute_force(x, g, y=None):
    """enumerate all A^T paths (NumPy float64): (Z_full, Z_tgt or None, best path, best score); the best path is the first
    maximum in lexicographic order of the REVERSED path, i.e. lowest final label, then lowest predecessor, ..."""
    x = np.asarray(x, dtype=np.float64)
    g = np.asarray(g, dtype=np.float64)
    T, A = x.shape
    scores, tgt = [], []
    best, best_path = -np.inf, None
    for rev in itertools.product(range(A), repeat=T):
        path = rev[::-1]
        s = path_score(x, g, path)
        scores.append(s)
        if y is not None and collapse(path) == list(y):
            tgt.append(s)
        if s > best:
            best, best_path = s, path
    lse = lambda v: float(np.max(v) + np.log(np.sum(np.exp(np.asarray(v) - np.max(v)))))      # noqa: E731
    return lse(scores), (lse(tgt) if tgt else None), list(best_path), float(best)


def viterbi(x, g):
    """best path of x [T, A] under transitions g: (path, score, margin).  Ties: lowest predecessor, lowest final label.
    margin = the smallest gap between a decision the path rests on and its runner-up (final label and every back-pointer
    on the path): a path with a margin above the fp32 error cannot be flipped by rounding."""
    x = np.asarray(x, dtype=np.float64)
    g = np.asarray(g, dtype=np.float64)
    T, A = x.shape
    score = x[0].copy()
    back = np.zeros((T, A), dtype=np.int64)
    gaps = np.full((T, A), np.inf)
    for t in range(1, T):
        cand = score[:, None] + g                      # [i, j]
        back[t] = np.argmax(cand, axis=0)              # first maximum: the lowest i
        if A > 1:
            top2 = np.sort(cand, axis=0)[-2:]
            gaps[t] = top2[1] - top2[0]
        score = x[t] + cand[back[t], np.arange(A)]
    last = int(np.argmax(score))
    margin = np.inf
    if A > 1:
        top2 = np.sort(score)[-2:]
        margin = top2[1] - top2[0]
    path = [last]
    for t in range(T - 1, 0, -1):
        margin = min(margin, gaps[t, path[-1]])
        path.append(int(back[t, path[-1]]))
    return path[::-1], float(score[last]), float(margin)


# ---- the float64 reference with per-element bounds (module docstring) ------------------------------------------------------------------

TCH = 64                   # frames per block of asg_grad_kernel
TP_MAX = 8192              # floats of its target-posterior buffer
K2_TGT = 2 * (HW_EXPF_ABS + 1 / math.e) + 2 + HW_LOGF_ABS
DEFECTS = ['grad_zero', 'stay_uses_adv', 'transposed_g', 'slab_skips_chunk_edge', 'state_window_off_by_one', 'repeat_parity',
           'second_state_slot_lost', 'mean_uses_encoded_gap', 'tail_not_zeroed']


def k2_full(A):
    return A * (HW_EXPF_ABS + 1 / math.e) + (A - 1) + (2 * HW_LOG + 2) * math.log(max(A, 3))


def asg_variant(A, Smax):
    """(AP, NT, SPT, dynamic LDS bytes of asg_grad_kernel): asg_plan of csrc/asg.hip restated"""
    ap = 32 if A <= 32 else 64
    sp = max(Smax, 1)
    nt = next((w for w in (64, 128, 256, 512, 1024) if sp <= w), 1024)
    spt = -(-sp // nt)
    if spt == 3:
        spt = 4
    tpn = min(TCH * sp, TP_MAX)
    return ap, nt, spt, ((2 * TCH + 1) * A + 3 * sp + tpn) * 4


def asg_workspace_bytes(N, T, A, Smax):
    sp = max(Smax, 1)
    return 4 * (2 * N * T * A + 2 * N * T * sp + N * sp + 2 * N + N * -(-T // TCH) * A * A)


def _encode(labels, repeat, defect=None):
    if defect != 'repeat_parity':
        return encode(labels, repeat)
    out, i = [], 0                                        # the defect: in a run of two or more, the 1st, 3rd, ... member is replaced
    while i < len(labels):
        j = i
        while j < len(labels) and labels[j] == labels[i]:
            j += 1
        out += [labels[i] if (j - i == 1 or (k - i) % 2) else repeat for k in range(i, j)]
        i = j
    return out


def _through_lse(p, d):
    """the error of a log-sum-exp whose arguments (weights p, summed over axis 0) are off by d: (module docstring)"""
    dmax = d.max(axis=0)
    return np.minimum(dmax, (np.minimum(1.0, p * np.exp(2 * dmax)) * d).sum(axis=0))


def _full_chain(x, G):
    """alpha_t(j) = x[t][j] + lse_i(alpha_{t-1}(i) + G[i][j]) over the rows of x [Tn][A] -> (alpha, E), both [Tn][A]; the beta chain
    is the same on time-reversed rows with G transposed"""
    Tn, A = x.shape
    al, E = np.empty((Tn, A)), np.zeros((Tn, A))
    al[0] = x[0]
    k2 = k2_full(A)
    for t in range(1, Tn):
        c = al[t - 1][:, None] + G
        m = c.max(axis=0)
        w = np.exp(c - m)
        s = w.sum(axis=0)
        em = x[t] + m
        v = em + np.log(s)
        al[t] = v
        E[t] = _through_lse(w / s, E[t - 1][:, None] + U * np.abs(c)) + U * (np.abs(em) + np.abs(v) + k2)
    return al, E


def _target_chain(x, y, stay, adv, kill_from=None):
    """alpha_t(s) = x[t][y_s] + lse2(alpha_{t-1}(s) + stay[s], alpha_{t-1}(s-1) + adv[s]) from state 0 at frame 0, over the states a
    path to state S-1 at the last frame can be in -> (alpha, E), both [Tn][S]: -inf and 0 elsewhere"""
    Tn, S = x.shape[0], len(y)
    al, E = np.full((Tn, S), -np.inf), np.zeros((Tn, S))
    al[0, 0] = x[0, y[0]]
    ninf, zero = np.full(1, -np.inf), np.zeros(1)
    for t in range(1, Tn):
        lo, hi = max(0, S - (Tn - t)), min(S - 1, t)
        a = al[t - 1, lo:hi + 1] + stay[lo:hi + 1]
        left = al[t - 1, lo - 1:hi] if lo > 0 else np.concatenate([ninf, al[t - 1, :hi]])
        eleft = E[t - 1, lo - 1:hi] if lo > 0 else np.concatenate([zero, E[t - 1, :hi]])
        b = left + adv[lo:hi + 1]
        lse = _lse(a, b)
        v = lse + x[t, y[lo:hi + 1]]
        if kill_from is not None:
            v[max(kill_from - lo, 0):] = -np.inf
        al[t, lo:hi + 1] = v
        with np.errstate(invalid='ignore'):
            fin = np.isfinite(v)
            ab = np.stack([a, b])
            p = np.where(np.isfinite(ab) & fin, np.exp(np.where(fin, ab - lse, 0.0)), 0.0)
            d = np.where(np.isfinite(ab), np.stack([E[t - 1, lo:hi + 1], eleft]) + U * np.abs(ab), 0.0)
            E[t, lo:hi + 1] = np.where(fin, _through_lse(p, d) + U * (np.abs(lse) + np.abs(v) + K2_TGT), 0.0)
    return al, E


def _exp_terms(u1, u2, u3, E0):
    """expf(u3) of an exponent reached through the sums u1, u2, u3 (one rounding each) from tables off by E0 in all:
    (terms, terms * expm1(E)); an exponent of -inf gives an exact 0"""
    with np.errstate(invalid='ignore', over='ignore'):
        fin = np.isfinite(u3)
        E = E0 + U * (np.abs(u1) + np.abs(u2) + np.abs(u3) + 2 * LIBM_EXPF + 2)
        term = np.where(fin, np.exp(np.where(fin, u3, 0.0)), 0.0)
        return term, np.where(fin, term * np.expm1(np.where(fin, E, 0.0)), 0.0)


def _utterance(x, g, y, Tn, want_grad, defect, kill_from):
    """one feasible utterance: x [Tn][A], encoded target y [S] -> dict of the unweighted pieces"""
    A = x.shape[1]
    S = len(y)
    G = g.T if defect == 'transposed_g' else g
    fa, Efa = _full_chain(x, G)
    m = fa[-1].max()
    w = np.exp(fa[-1] - m)
    s = float(w.sum())
    zf = float(m + math.log(s))
    Ezf = float(_through_lse(w / s, Efa[-1])) + U * (A / math.e + 2 * LIBM_EXPF + 6 + 2 * LIBM_LOGF * math.log(s) + abs(zf) + 2)
    stay = g[y, y].copy()
    adv = np.concatenate([[0.0], g[y[:-1], y[1:]]])         # adv[s] = g[y_{s-1}][y_s]; adv[0] is never used
    if defect == 'stay_uses_adv':
        stay[1:] = adv[1:]
    ta, Eta = _target_chain(x, y, stay, adv, kill_from)
    zt, Ezt = float(ta[-1, S - 1]), float(Eta[-1, S - 1])
    out = dict(nll=zf - zt, nll_b=Ezf + Ezt + U * abs(zf - zt))
    if not np.isfinite(zt) or not want_grad:
        return out
    fb_r, Efb_r = _full_chain(x[::-1], G.T)
    fb, Efb = fb_r[::-1], Efb_r[::-1]
    adv_r = np.concatenate([[0.0], adv[1:][::-1]])
    tb_r, Etb_r = _target_chain(x[::-1], y[::-1], stay[::-1], adv_r)
    tb, Etb = tb_r[::-1, ::-1], Etb_r[::-1, ::-1]
    # emissions: the full posterior, every frame at once
    ab = fa + fb
    pf, pfb = _exp_terms(ab, ab - x, ab - x - zf, Efa + Efb + Ezf)
    # pairs of the full recursion, frames 1 .. Tn-1
    keep = np.ones(Tn, dtype=bool)
    keep[0] = False
    if defect == 'slab_skips_chunk_edge':
        keep[TCH::TCH] = False
    ts = np.nonzero(keep)[0]
    F, Fb = np.zeros((A, A)), np.zeros((A, A))
    for k in range(0, len(ts), 256):
        tt = ts[k:k + 256]
        u1 = fa[tt - 1][:, :, None] + G[None]
        u2 = u1 + fb[tt][:, None, :]
        term, tb_ = _exp_terms(u1, u2, u2 - zf, Efa[tt - 1][:, :, None] + Efb[tt][:, None, :] + Ezf)
        F += term.sum(axis=0)
        Fb += tb_.sum(axis=0)
    # the target's posteriors, frame by frame over the states a path can be in
    pt, ptb = np.zeros((Tn, A)), np.zeros((Tn, A))
    Tp, Tpb = np.zeros(A * A), np.zeros(A * A)
    yprev = np.concatenate([[0], y[:-1]])
    ninf, zero = np.full(1, -np.inf), np.zeros(1)
    for t in range(Tn):
        lo, hi = max(0, S - (Tn - t)), min(S - 1, t)
        if keep[t]:
            b, eb = tb[t, lo:hi + 1], Etb[t, lo:hi + 1] + Ezt
            ys = y[lo:hi + 1]
            u1 = ta[t - 1, lo:hi + 1] + stay[lo:hi + 1]
            term, tb_ = _exp_terms(u1, u1 + b, u1 + b - zt, Eta[t - 1, lo:hi + 1] + eb)
            Tp += np.bincount(ys * A + ys, weights=term, minlength=A * A)
            Tpb += np.bincount(ys * A + ys, weights=tb_, minlength=A * A)
            left = ta[t - 1, lo - 1:hi] if lo > 0 else np.concatenate([ninf, ta[t - 1, :hi]])
            eleft = Eta[t - 1, lo - 1:hi] if lo > 0 else np.concatenate([zero, Eta[t - 1, :hi]])
            u1 = left + adv[lo:hi + 1]
            term, tb_ = _exp_terms(u1, u1 + b, u1 + b - zt, eleft + eb)
            Tp += np.bincount(yprev[lo:hi + 1] * A + ys, weights=term, minlength=A * A)
            Tpb += np.bincount(yprev[lo:hi + 1] * A + ys, weights=tb_, minlength=A * A)
        if defect == 'state_window_off_by_one':
            lo, hi = lo + 1, min(hi + 1, S - 1)
            if lo > hi:
                continue
        ys = y[lo:hi + 1]
        v = ta[t, lo:hi + 1] + tb[t, lo:hi + 1]
        tp, tpb = _exp_terms(v, v - x[t, ys], v - x[t, ys] - zt, Eta[t, lo:hi + 1] + Etb[t, lo:hi + 1] + Ezt)
        cnt = np.bincount(ys, minlength=A)
        pt[t] = np.bincount(ys, weights=tp, minlength=A)
        ptb[t] = np.bincount(ys, weights=tpb, minlength=A) + np.maximum(cnt - 1, 0) * U * pt[t]
    Tp, Tpb = Tp.reshape(A, A), Tpb.reshape(A, A)
    nm = (np.bincount(y * A + y, minlength=A * A) + np.bincount(yprev[1:] * A + y[1:], minlength=A * A)).reshape(A, A)
    out.update(gx=pf - pt, gxb=pfb + ptb + 6 * U * (pf + pt), D=F - Tp, B=Fb + Tpb + (TCH - 1 + nm + 6) * U * (F + Tp), M=F + Tp)
    return out


def asg_ref(x, g, targets, in_len, tg_len, repeat, reduction, Smax, want_grad=True, defect=None):
    """x [N][T][A] and g [A][A] fp32 values, targets [N][Smax] RAW transcripts, in_len / tg_len [N] as the caller passes them.
    Returns a dict: nll, nll_b [N]; loss, loss_b; grad_x, grad_x_b [N][T][A]; grad_g, grad_g_b [A][A]; status [N]; S, Tn (clamped)."""
    return asg_reduce(asg_parts(x, g, targets, in_len, tg_len, repeat, Smax, want_grad, defect), reduction, defect)


def asg_parts(x, g, targets, in_len, tg_len, repeat, Smax, want_grad=True, defect=None):
    """everything of asg_ref that does not depend on the reduction"""
    x = np.asarray(x, dtype=np.float64)
    g = np.asarray(g, dtype=np.float64)
    N, T, A = x.shape
    Ss = np.clip(np.asarray(tg_len, dtype=np.int64), 0, Smax)
    Tns = np.clip(np.asarray(in_len, dtype=np.int64), 0, T)
    _, nt, spt, _ = asg_variant(A, Smax)
    kill_from = nt if (defect == 'second_state_slot_lost' and spt > 1) else None
    P = dict(N=N, T=T, A=A, S=Ss, Tn=Tns, Sw=Ss.copy(), status=np.zeros(N, dtype=np.int32), nll=np.zeros(N), nll_b=np.zeros(N),
             gx=np.zeros((N, T, A)), gxb=np.zeros((N, T, A)), D=np.zeros((N, A, A)), B=np.zeros((N, A, A)), M=np.zeros((N, A, A)),
             want_grad=want_grad, x=x)
    for n in range(N):
        S, Tn = int(Ss[n]), int(Tns[n])
        raw = [int(v) for v in np.asarray(targets)[n, :S]] if S else []
        if any(v < 0 or v >= A or v == repeat for v in raw):
            P['status'][n] = 2
            continue
        if S == 0 or S > Tn:
            P['status'][n] = 1
            continue
        y = np.array(_encode(raw, repeat, defect), dtype=np.int64)
        P['Sw'][n] = int((y != repeat).sum())                # what the defect 'mean_uses_encoded_gap' divides by
        u = _utterance(x[n, :Tn], g, y, Tn, want_grad, defect, kill_from)
        P['nll'][n], P['nll_b'][n] = u['nll'], u['nll_b']
        if not np.isfinite(u['nll']):
            P['gx'][n], P['D'][n] = np.nan, np.nan
        elif want_grad:
            P['gx'][n, :Tn], P['gxb'][n, :Tn] = u['gx'], u['gxb'] + (S + 2) * TINY
            P['D'][n], P['B'][n], P['M'][n] = u['D'], u['B'] + Tn * (S + 2) * TINY, u['M']
    return P


def asg_reduce(P, reduction, defect=None):
    N, T = P['N'], P['T']
    ok = P['status'] == 0
    Sw = P['Sw'] if defect == 'mean_uses_encoded_gap' else P['S']
    mean = reduction == 'mean'
    w = np.where(ok, 1.0 / (N * np.maximum(Sw, 1)) if mean else 1.0, 0.0)
    with np.errstate(invalid='ignore'):
        terms = P['nll'] * (w * N if mean else w)
        loss = terms.sum() / N if mean else terms.sum()
        # a quotient per utterance ('mean'), N additions in order, the division by N
        fin = np.isfinite(terms)
        loss_b = (P['nll_b'] * (w if mean else 1.0)).sum() + (N + 2 + 2) * U * np.abs(terms[fin]).sum() / (N if mean else 1)
    out = dict(nll=P['nll'].copy(), nll_b=P['nll_b'].copy(), loss=float(loss), loss_b=float(loss_b), status=P['status'].copy(),
               S=P['S'], Tn=P['Tn'])
    if not P['want_grad']:
        return out
    chunks = -(-T // TCH)
    with np.errstate(invalid='ignore'):
        gx = P['gx'] * w[:, None, None]
        gxb = P['gxb'] * w[:, None, None]
        gg = (P['D'] * w[:, None, None]).sum(axis=0)
        ggb = (P['B'] * w[:, None, None]).sum(axis=0) + (N * chunks + 1) * U * (P['M'] * w[:, None, None]).sum(axis=0)
    if defect == 'grad_zero':
        gx = np.zeros_like(gx)
    if defect == 'tail_not_zeroed':
        for n in range(N):
            gx[n, P['Tn'][n]:] = np.exp(np.minimum(P['x'][n, P['Tn'][n]:], 0.0)) * max(w[n], 1.0 / N)
    out.update(grad_x=gx, grad_x_b=gxb, grad_g=gg, grad_g_b=ggb)
    return out


# ---- the cases the CPU and the GPU tests share ------------------------------------------------------------------------------------

@dataclasses.dataclass(frozen=True, eq=False)
class AsgCase:
    name: str
    x: np.ndarray              # [N][T][A] fp32
    g: np.ndarray              # [A][A] fp32
    targets: np.ndarray        # [N][max(Smax, 1)] int32 raw transcripts, padded with -7 (never a valid label, never read)
    in_len: np.ndarray
    tg_len: np.ndarray
    Smax: int
    repeat: int = 0

    @property
    def dims(self):
        return self.x.shape

    @property
    def variant(self):
        return asg_variant(self.x.shape[2], self.Smax)


BOUNDARIES = (64, 128, 256, 512, 1024, 2048, 3072)


def _raw(rng, S, A, repeat=0):
    """S raw labels; a run of four equal letters across every thread-count boundary below S (states b-2 .. b+1)"""
    labs = [v for v in range(A) if v != repeat]
    t = [int(v) for v in rng.choice(labs, size=S)] if S else []
    for b in BOUNDARIES:
        if b + 2 <= S:
            t[b - 2:b + 2] = [t[b - 2]] * 4
    return t


def _log_softmax(a):
    a = a - a.max(axis=-1, keepdims=True)
    return a - np.log(np.exp(a).sum(axis=-1, keepdims=True))


def make_case(name, rng, A, T, rows, in_len, Smax, repeat=0, tg_len=None):
    """rows: raw transcripts.  T <= 300: random log-probabilities and standard-normal transitions.  Longer: the emissions of a drawn
    feasible alignment (its label near 0, the rest well below) and small transitions, which keep the log-domain magnitudes, and so
    the bound, small."""
    N = len(rows)
    tg = np.full((N, max(Smax, 1)), -7, dtype=np.int32)
    for n, r in enumerate(rows):
        tg[n, :min(len(r), Smax)] = r[:Smax]
    tg_len = [len(r) for r in rows] if tg_len is None else tg_len
    if T <= 300:
        x = _log_softmax(3.0 * rng.standard_normal((N, T, A)))
        g = rng.standard_normal((A, A))
    else:
        x = -5.0 - 2.0 * rng.random((N, T, A))
        g = 0.1 * rng.standard_normal((A, A))
        for n, r in enumerate(rows):
            Tn, S = max(0, min(int(in_len[n]), T)), min(len(r), Smax)
            lab = rng.integers(0, A, size=T)
            if 0 < S <= Tn and all(0 <= v < A and v != repeat for v in r[:S]):
                state = np.zeros(Tn, dtype=np.int64)
                state[np.sort(rng.choice(Tn - 1, size=S - 1, replace=False)) + 1] = 1
                lab[:Tn] = np.array(encode(r[:S], repeat))[np.cumsum(state)]
            x[n, np.arange(T), lab] = -0.01 * rng.random(T)
    return AsgCase(name, x.astype(np.float32), g.astype(np.float32), tg, np.asarray(in_len, dtype=np.int32),
                   np.asarray(tg_len, dtype=np.int32), Smax, repeat)


def _labels_case(A):
    rng = np.random.default_rng(8000 + A)
    if A == 1:                                               # the only label is the repeat label: nothing is feasible
        return make_case('A1', rng, 1, 12, [[0, 0], [], [0]], [12, 12, 5], 2)
    rows = [_raw(rng, 12, A), [1, 1, 2, 2, 2, A - 1], _raw(rng, 1, A), [A - 1] * 4 + [1] * 5]
    return make_case(f'A{A}', rng, A, 12, rows, [12, 12, 1, 10], 12)


def _width_case(Smax):
    """one utterance of S = Smax in T = S + 6 frames, one short, one infeasible (S > Tn), one empty"""
    rng = np.random.default_rng(8100 + Smax)
    T = Smax + 6
    rows = [_raw(rng, Smax, 5), _raw(rng, 7, 5), _raw(rng, 9, 5), []]
    return make_case(f'S{Smax}', rng, 5, T, rows, [T, T - 3, 8, T], Smax)


def _spt_case(Smax):
    rng = np.random.default_rng(8200 + Smax)
    return make_case(f'S{Smax}', rng, 5, Smax + 6, [_raw(rng, Smax, 5)], [Smax + 6], Smax)


def _wide_pad_case(A, Smax, T, lens, name):
    """few states under a padded Smax: the padded width alone picks the kernel and the LDS size"""
    rng = np.random.default_rng(8300 + A + Smax)
    rows = [_raw(rng, s, A) for s in lens]
    return make_case(name, rng, A, T, rows, [T - 2 * n for n in range(len(lens))], Smax)


def _frames_case(T):
    rng = np.random.default_rng(8400 + T)
    rows = [_raw(rng, 9, 5), [1, 1, 1, 2], _raw(rng, 30, 5), [3], [2]]
    return make_case(f'T{T}', rng, 5, T, rows, [T, 64, 63, 1, 0], 30)


def _passes_case(S):
    rng = np.random.default_rng(8500 + S)
    return make_case(f'fb{S}', rng, 5, 140, [_raw(rng, S, 5)], [140], S)


def _runs_case():
    rng = np.random.default_rng(8600)
    rows = [[1, 1, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 4], [2] * 5 + [1] * 2, [3] * 24, [4, 4, 1, 4, 4]]
    return make_case('runs', rng, 5, 26, rows, [26, 20, 24, 26], 24)


def _bad_case(kind, repeat):
    A = 6
    rng = np.random.default_rng(8700 + 10 * repeat + len(kind))
    bad = {'negative': -1, 'A': A, 'repeat': repeat}[kind]
    ok = [v for v in range(A) if v != repeat]
    rows = [[ok[0], ok[0], ok[1], ok[2]], [ok[1], bad, ok[3]], [ok[4], ok[4], ok[4]]]
    return make_case(f'bad-{kind}-r{repeat}', rng, A, 10, rows, [10, 10, 9], 4, repeat)


def _clamp_case():
    """tg_len above Smax (read as Smax), in_len above T (read as T) and negative (read as 0: infeasible)"""
    rng = np.random.default_rng(8800)
    rows = [_raw(rng, 6, 5), _raw(rng, 4, 5), _raw(rng, 3, 5)]
    return make_case('clamps', rng, 5, 14, rows, [14, 99, -3], 6, tg_len=[9, 4, 3])


WIDTHS = (64, 65, 128, 129, 256, 257, 512, 513, 1024)
SPT_WIDTHS = (1025, 2048, 2049, 3073, 4095)
CASES = {}
for _A in (1, 5, 32, 33, 64):
    CASES[f'A{_A}'] = functools.partial(_labels_case, _A)
for _S in WIDTHS:
    CASES[f'S{_S}'] = functools.partial(_width_case, _S)
for _S in SPT_WIDTHS:
    CASES[f'S{_S}'] = functools.partial(_spt_case, _S)
CASES['A64-S4095'] = functools.partial(_wide_pad_case, 64, 4095, 70, (20, 9), 'A64-S4095')
CASES['A64-S513'] = functools.partial(_wide_pad_case, 64, 513, 130, (100, 40), 'A64-S513')
for _S in (100, 200, 400, 1500):                             # AP = 64 with every remaining block shape
    CASES[f'A33-S{_S}'] = functools.partial(_wide_pad_case, 33, _S, 12, (10, 5), f'A33-S{_S}')
for _T in (64, 65, 128, 129):
    CASES[f'T{_T}'] = functools.partial(_frames_case, _T)
for _S in (127, 128, 129):
    CASES[f'fb{_S}'] = functools.partial(_passes_case, _S)
CASES['runs'] = _runs_case
for _kind in ('negative', 'A', 'repeat'):
    for _r in (0, 5):
        CASES[f'bad-{_kind}-r{_r}'] = functools.partial(_bad_case, _kind, _r)
CASES['clamps'] = _clamp_case
LONG = [k for k in CASES if k.startswith('S') and int(k[1:]) + 6 > 300]

VITERBI_A = (1, 5, 32, 33, 64)
VITERBI_T = (1, 2, 511, 512, 513, 1024, 1025)                # around the 512-frame chunks of the back-trace


@functools.lru_cache(maxsize=None)
def viterbi_case(A, T):
    """x [4][T][A] and g [A][A] of small integers: every partial sum is exact in fp32, so ties are exact and frequent.  Labels 0
    and 1 tie at frame 0 with the largest value and leave with the same transitions: a tie of the final label at T = 1, of the
    predecessor after.  Input lengths T, 0, 1 and one below T.  -> (x, g, in_len, [(path, score, margin) per utterance] under
    in_len, the same with every utterance T frames long)"""
    rng = np.random.default_rng(9000 + 100 * A + T)
    x = rng.integers(-3, 4, size=(4, T, A)).astype(np.float32)
    g = rng.integers(-3, 4, size=(A, A)).astype(np.float32)
    if A > 1:
        x[:, 0, :2] = 3.0
        g[1] = 3.0 if T <= 2 else g[0]                       # (two frames: the one step must tie, so both leave with the largest value)
        g[0] = g[1]
    in_len = np.array([T, 0, 1, max(T - 3, 1)], dtype=np.int32)
    refs = [viterbi(x[n, :tn], g) if tn else ([], 0.0, np.inf) for n, tn in enumerate(in_len)]
    return x, g, in_len, refs, [viterbi(x[n], g) for n in range(4)]


ENGLISH = "_'abcdefghijklmnopqrstuvwxyz "


def old_pad(targets):
    smax = max(1, max(len(t) for t in targets))
    tg = np.zeros((len(targets), smax), dtype=np.int32)
    for n, t in enumerate(targets):
        tg[n, :len(t)] = t
    return tg, np.array([len(t) for t in targets], dtype=np.int32)


def old_case(name):
    """the cases test_gpu_asg.py has had from the start: (x [N, T, A] float32, g [A, A] float32, raw transcripts, output lengths)"""
    seed = {'main': 0, 'a29': 1, 'a33': 2, 'chunks': 3, 'long': 4, 'spt2': 5}[name]
    rng = np.random.default_rng(100 + seed)
    if name == 'main':
        N, T, A = 5, 12, 5
        lens = [12, 12, 7, 1, 3]
        targets = [rng.integers(1, A, 3).tolist(), rng.integers(1, A, 12).tolist(), [2, 3, 3, 1], [4],
                   rng.integers(1, A, 5).tolist()]
    elif name == 'a29':
        N, T, A = 3, 40, 29
        lens = [40, 33, 25]
        targets = [[ENGLISH.index(c) for c in s] for s in ('hello world', "see the bookkeeper's", 'a')]
    elif name == 'a33':
        N, T, A = 2, 10, 33
        lens = [10, 8]
        targets = [rng.integers(1, A, 4).tolist(), [32, 32, 32, 7, 1, 1, 20]]
    elif name == 'chunks':
        N, T, A = 2, 70, 5
        lens = [70, 66]
        targets = [rng.integers(1, A, 9).tolist(), rng.integers(1, A, 65).tolist()]
    elif name == 'long':
        N, T, A = 1, 140, 5
        lens = [140]
        targets = [rng.integers(1, A, 130).tolist()]
    else:
        N, T, A = 1, 1100, 5
        lens = [1100]
        targets = [rng.integers(1, A, 1030).tolist()]
    x = _log_softmax(3.0 * rng.standard_normal((N, T, A))).astype(np.float32)
    g = rng.standard_normal((A, A)).astype(np.float32)
    return x, g, targets, lens


def old_case_ref(name, reduction, scale=(1.0, 1.0)):
    """asg_ref (with its bounds) of an old case, emissions and transitions scaled as test_large_dynamic_range scales them"""
    x, g, targets, lens = old_case(name)
    x, g = x * np.float32(scale[0]), g * np.float32(scale[1])
    tg, tl = old_pad(targets)
    return asg_ref(x, g, tg, lens, tl, 0, reduction, tg.shape[1])


_CASE_CACHE, _PARTS_CACHE = {}, {}


def case(name):
    if name not in _CASE_CACHE:
        _CASE_CACHE[name] = CASES[name]()
    return _CASE_CACHE[name]


def case_ref(name, reduction, defect=None):
    """the reference of a shared case; what does not depend on the reduction is computed once per session (a defective one is kept
    only where the defect acts in the reduction)"""
    c = case(name)
    late = defect in (None, 'grad_zero', 'mean_uses_encoded_gap', 'tail_not_zeroed')
    if late:
        if name not in _PARTS_CACHE:
            _PARTS_CACHE[name] = asg_parts(c.x, c.g, c.targets, c.in_len, c.tg_len, c.repeat, c.Smax)
        return asg_reduce(_PARTS_CACHE[name], reduction, defect)
    return asg_ref(c.x, c.g, c.targets, c.in_len, c.tg_len, c.repeat, reduction, c.Smax, defect=defect)
