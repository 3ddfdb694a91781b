"""References for the CTC keyword search (wav2letter_pytorch_amd/keyword_search.py, csrc/ctc_kws.hip), written apart from the
package's own host model: the scan in float64 with scalar loops, the brute force it is checked against (every slice [t0, t1]
through alignment.viterbi_align_host with the blank forbidden on the slice's first and last frame), the pick rule, and the
inputs the tests share.

The error bound of the fp32 scan.  With u = 2^-24: in max-plus arithmetic a max selects one of its arguments and adds no error,
so the error of D[t][s] is the error accumulated along ONE path.  Along a path every frame does one subtraction e = lp - b
(inputs exact, error <= u |e|) and one addition D' = D + e (error <= u |D'|).  All e are <= 0, so |D| grows along the path and
sum |e| = |D|; after Tn frames the accumulated error is at most Tn u |D| + u |D| <= (Tn + 1) u P with P the largest finite
magnitude of the keyword's float64 table.  The fp32 maximum may pick another path than the fp64 one; it then differs from the
fp64 maximum by no more than the error of the two paths' scores, which the same bound covers with one more u P of slack:

    |D32 - D64| <= (Tn + 2) * 2^-24 * P

test_cpu_keyword_search.py checks it on the host (fp32 against fp64 model); test_gpu_keyword_search.py holds the device to it.
With probabilities as input the device forms e = logf(x) - logf(b), and the two logf roundings are an error this derivation
does not budget for; the device tests hold that mode to the same bound all the same (measured on the MI355X: at most 0.93 of
it, at T = 1 where those roundings are the whole error; log-probabilities: at most 0.21)."""
import numpy as np

NINF = float('-inf')
DEFECTS = ('twin_skip', 'enter_first', 'no_b', 'enter_blank')


def kws_bound(t_n, p):
    return (t_n + 2) * 2.0 ** -24 * p


def scan_ref(lp, keyword, blank=0, length=None, defect=None):
    """float64, scalar loops -> dict(end_score [T], end_start [T], P = the largest finite |D| of the table).  ``defect`` plants
    one of DEFECTS (the tests show that each is caught)."""
    lp = np.asarray(lp, dtype=np.float64)
    T, A = lp.shape
    kw = [int(v) for v in keyword]
    S = len(kw)
    assert S >= 1 and all(0 <= v < A and v != blank for v in kw)
    Tn = T if length is None else min(max(int(length), 0), T)
    L = 2 * S - 1
    lab = [kw[s >> 1] if s % 2 == 0 else blank for s in range(L)]
    skip = [s % 2 == 0 and s >= 2 and (kw[s >> 1] != kw[(s >> 1) - 1] or defect == 'twin_skip') for s in range(L)]
    D = [NINF] * L
    B = [-1] * L
    end_score = np.full(T, NINF)
    end_start = np.full(T, -1, dtype=np.int64)
    P = 0.0
    for t in range(Tn):
        b = 0.0 if defect == 'no_b' else float(lp[t].max())
        nd, nb = [NINF] * L, [-1] * L
        for s in range(L):
            cands = [(D[s], B[s])]
            if s >= 1:
                cands.append((D[s - 1], B[s - 1]))
            if s >= 2 and skip[s]:
                cands.append((D[s - 2], B[s - 2]))
            if s == 0 or (defect == 'enter_blank' and s == 1):
                if defect == 'enter_first':
                    cands.insert(0, (0.0, t))
                else:
                    cands.append((0.0, t))
            best, bb = cands[0]
            for v, f in cands[1:]:
                if v > best:
                    best, bb = v, f
            v = best + (float(lp[t, lab[s]]) - b) if best > NINF else NINF
            if v > NINF:
                nd[s], nb[s] = v, bb
                P = max(P, abs(v))
        D, B = nd, nb
        end_score[t], end_start[t] = D[L - 1], B[L - 1]
    return dict(end_score=end_score, end_start=end_start, P=P)


def slice_score(lp, keyword, t0, t1, blank=0):
    """the float64 forced alignment of the keyword within frames [t0, t1] of lp, normalised by the frame maxima, the blank
    forbidden on the slice's first and last frame -> score (-inf if infeasible)"""
    from wav2letter_pytorch_amd.alignment import viterbi_align_host
    lp = np.asarray(lp, dtype=np.float64)
    piece = lp[t0: t1 + 1] - lp[t0: t1 + 1].max(axis=1, keepdims=True)
    piece[0, blank] = NINF
    piece[-1, blank] = NINF
    return float(viterbi_align_host(piece, keyword, blank=blank).score)


def brute_force(lp, keyword, blank=0):
    """every slice -> (end_score [T], end_start [T] (the EARLIEST best start), unique [T]: the best start is the only one)"""
    T = len(lp)
    end_score = np.full(T, NINF)
    end_start = np.full(T, -1, dtype=np.int64)
    unique = np.zeros(T, dtype=bool)
    for t1 in range(T):
        scores = [slice_score(lp, keyword, t0, t1, blank) for t0 in range(t1 + 1)]
        best = max(scores)
        if best > NINF:
            end_score[t1] = best
            end_start[t1] = scores.index(best)
            unique[t1] = scores.count(best) == 1
    return end_score, end_start, unique


def pick_ref(end_score, end_start, thr, max_hits):
    """the pick rule, written as the search it describes: repeat -- best free candidate by (score desc, start asc, end desc)"""
    accepted = []
    for _ in range(max_hits):
        best = None
        for t in range(len(end_score)):
            sc, st = end_score[t], int(end_start[t])
            if not sc >= thr or st < 0:
                continue
            if any(st <= e and s <= t for s, e, _ in accepted):
                continue
            key = (-float(sc), st, -t)
            if best is None or key < best[0]:
                best = (key, (st, t, float(sc)))
        if best is None:
            break
        accepted.append(best[1])
    return sorted(accepted)


# ---------------------------------------------------------------------------------------------------------------- inputs
def random_lp(seed, T, A, ninf_fraction=0.0, dtype=np.float32):
    """log-softmax of random logits, rounded to ``dtype``; with ``ninf_fraction`` that share of the entries is -inf (never a
    whole frame)"""
    g = np.random.default_rng(seed)
    z = 2.0 * g.standard_normal((T, A))
    lp = z - np.log(np.exp(z).sum(axis=1, keepdims=True))
    if ninf_fraction:
        hole = g.random((T, A)) < ninf_fraction
        hole[np.arange(T), lp.argmax(axis=1)] = False
        lp[hole] = NINF
    return lp.astype(dtype)


def planted_lp(seed, T, A, frame_path, dtype=np.float32):
    """random logits with +8 on the label of a hand-written frame path {frame: label}: the path's labels are the frames'
    argmax, so a keyword it spells scores exactly 0 there"""
    g = np.random.default_rng(seed)
    z = g.standard_normal((T, A))
    for t, a in frame_path.items():
        z[t, a] += 8.0
    lp = (z - np.log(np.exp(z).sum(axis=1, keepdims=True))).astype(dtype)
    for t, a in frame_path.items():
        assert lp[t].argmax() == a and (lp[t] == lp[t, a]).sum() == 1
    return lp


def path_of(spans):
    """[(label, first frame, last frame), ...] -> {frame: label}"""
    return {t: a for a, t0, t1 in spans for t in range(t0, t1 + 1)}


# keyword [2, 3, 3, 1] (a doubled letter: the blank between the twins is required) said twice in 40 frames, blank = 0; every
# other frame of the neighbourhood is a planted blank, so the greedy path spells the keyword on exactly these frames
PLANTED_KW = [2, 3, 3, 1]
PLANTED_SPANS = [(0, 0, 2), (2, 3, 4), (3, 5, 5), (0, 6, 7), (3, 8, 9), (0, 10, 10), (1, 11, 13), (0, 14, 19),
                 (2, 20, 20), (3, 21, 22), (0, 23, 23), (3, 24, 24), (1, 25, 27), (0, 28, 31)]
PLANTED_SEGMENTS = [(3, 13), (20, 27)]
