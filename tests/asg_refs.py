"""Float64 references of the ASG criterion and its Viterbi decoder (torch on the CPU, NumPy), written from the definitions:

  Z_full = logsumexp over all A^T frame paths of  sum_t x[t, pi_t] + sum_{t>=1} g[pi_{t-1}, pi_t]
  Z_tgt  = the same over the paths that read the encoded target y, every label held for at least one frame
  loss   = Z_full - Z_tgt

``full_logz`` / ``target_logz`` are the two recursions as plain torch.logsumexp loops (autograd gives the gradients);
``brute_force`` enumerates every path and pins those recursions; ``viterbi`` is the best path with ties to the lowest
predecessor and the lowest final label."""
import itertools

import numpy as np
import torch


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
