"""Plain numpy restatement of the segmentation rule (DESIGN.md "Long-form transcription"; csrc/vad.hip implements it on the
device): sequential loops over frames and runs, nothing shared with the kernel's structure (no scans, no radix select, no
tiles).  All index ranges are half-open.

``defect=`` plants one wrong reading of the rule, to show that the test inputs tell it from the right one:
  'on_gt'            P > thr_on instead of P >= thr_on
  'off_le'           P <= thr_off instead of P < thr_off
  'close_drop_swap'  short runs are dropped before gaps are closed
  'gap_off_by_one'   a gap of exactly min_silence is closed too
  'last_min'         the forced cut takes the last of equal minima
  'carry_1024'       the hysteresis state is forgotten at every multiple of 1024 frames
  'partial_own_len'  a partial last frame is divided by its own length instead of win
"""
import math

import numpy as np

DEFECTS = ('on_gt', 'off_le', 'close_drop_swap', 'gap_off_by_one', 'last_min', 'carry_1024', 'partial_own_len')


def frame_sums(x, win, hop):
    """fp64 sums of squares per frame, added one sample after the other, and the number of samples of each frame"""
    x = np.asarray(x, dtype=np.float32).reshape(-1)
    n = x.shape[0]
    F = -(-n // hop)
    xd = np.concatenate([x.astype(np.float64), np.zeros(win, dtype=np.float64)])      # (+0.0 past the end adds nothing)
    start = np.arange(F, dtype=np.int64) * hop
    counts = np.minimum(n, start + win) - start
    sums = np.zeros(F, dtype=np.float64)
    for i in range(win):                                 # sample after sample, every frame at once
        v = xd[start + i]
        sums = sums + v * v
    return sums, counts


def frame_power(x, win, hop, defect=None):
    sums, counts = frame_sums(x, win, hop)
    div = counts.astype(np.float64) if defect == 'partial_own_len' else float(win)
    return (sums / div).astype(np.float32)


def clean(P):
    """the powers as every decision reads them (NaN and negative values count as 0) and status bit 1"""
    P = np.asarray(P, dtype=np.float32).reshape(-1)
    bad = ~(P >= 0)
    out = np.where(bad, np.float32(0), P) + np.float32(0)           # (-0 + 0 = +0)
    return out.astype(np.float32), (2 if bad.any() else 0)


def statistics(P, q):
    """(floor, peak) as float32: the floor(q (F - 1))-th smallest power and the largest"""
    P, _ = clean(P)
    if P.shape[0] == 0:
        return np.float32(0), np.float32(0)
    k = int(math.floor(q * (P.shape[0] - 1)))
    k = min(max(k, 0), P.shape[0] - 1)
    return np.sort(P, kind='stable')[k], P.max()


def thresholds(floor, peak, r_on, r_hyst, abs_min):
    """adaptive thresholds, in Python floats (fp64) from the fp32 statistics"""
    fl, pk = float(floor), float(peak)
    on = max(abs_min, min(fl * r_on, math.sqrt(fl * pk)))
    return on, on * r_hyst


def hysteresis(P, thr_on, thr_off, defect=None):
    s = np.zeros(len(P), dtype=np.int8)
    prev = 0
    for f, pw in enumerate(P):
        pw = float(pw)
        if defect == 'carry_1024' and f > 0 and f % 1024 == 0:
            prev = 0
        on = pw > thr_on if defect == 'on_gt' else pw >= thr_on
        off = pw <= thr_off if defect == 'off_le' else pw < thr_off
        if on:
            prev = 1
        elif off:
            prev = 0
        s[f] = prev
    return s


def runs_of(s):
    runs, a = [], None
    for f, v in enumerate(s):
        if v and a is None:
            a = f
        if not v and a is not None:
            runs.append((a, f))
            a = None
    if a is not None:
        runs.append((a, len(s)))
    return runs


def close_gaps(runs, min_silence, defect=None):
    out = []
    for a, b in runs:
        gap_closes = out and ((a - out[-1][1] <= min_silence) if defect == 'gap_off_by_one' else (a - out[-1][1] < min_silence))
        if gap_closes:
            out[-1] = (out[-1][0], b)
        else:
            out.append((a, b))
    return out


def drop_short(runs, min_speech):
    return [(a, b) for a, b in runs if b - a >= min_speech]


def pad_merge(runs, pad, F):
    out = []
    for a, b in runs:
        a, b = max(0, a - pad), min(F, b + pad)
        if out and a <= out[-1][1]:
            out[-1] = (out[-1][0], b)
        else:
            out.append((a, b))
    return out


def forced_split(runs, P, max_frames, defect=None):
    h = max_frames // 2
    out = []
    for a, b in runs:
        while b - a > max_frames:
            lo, hi = a + h, min(a + max_frames, b - h)
            assert lo < hi
            c, best = lo, P[lo]
            for i in range(lo + 1, hi):
                if P[i] < best or (defect == 'last_min' and P[i] == best):
                    c, best = i, P[i]
            out.append((a, c))
            a = c
        out.append((a, b))
    return out


def decide(P, thr_on, thr_off, min_silence, min_speech, pad, max_frames, defect=None):
    """the segments in frames from the powers and the two thresholds"""
    P, _ = clean(P)
    runs = runs_of(hysteresis(P, thr_on, thr_off, defect))
    if defect == 'close_drop_swap':
        runs = close_gaps(drop_short(runs, min_speech), min_silence, defect)
    else:
        runs = drop_short(close_gaps(runs, min_silence, defect), min_speech)
    runs = pad_merge(runs, pad, len(P))
    return forced_split(runs, P, max_frames, defect)


def segment(P, *, q=0.05, r_on=10.0, r_hyst=10 ** -0.3, abs_min=1e-10, thr_on=None, thr_off=None, min_silence=30, min_speech=10,
            pad=20, max_frames=2000, cap=None, defect=None):
    """the whole decision pass on a power array -> dict(count, status, thr_on, thr_off, floor, peak, segments); absolute mode
    when ``thr_on`` is given (``thr_off`` with it)"""
    Pc, status = clean(P)
    floor, peak = statistics(Pc, q)
    if thr_on is None:
        thr_on, thr_off = thresholds(floor, peak, r_on, r_hyst, abs_min)
    segs = decide(Pc, thr_on, thr_off, min_silence, min_speech, pad, max_frames, defect)
    count = len(segs)
    if cap is not None and count > cap:
        status |= 1
        segs = segs[:cap]
    return dict(count=count, status=status, thr_on=thr_on, thr_off=thr_off, floor=floor, peak=peak,
                segments=np.asarray(segs, dtype=np.int64).reshape(-1, 2))


def to_samples(segs, hop, n):
    segs = np.asarray(segs, dtype=np.int64).reshape(-1, 2)
    return np.stack([segs[:, 0] * hop, np.minimum(n, segs[:, 1] * hop)], 1) if len(segs) else segs


def vad_reference(x, win, hop, defect=None, **kw):
    """from the waveform: frame powers, then ``segment``; segments in samples under 'samples'"""
    P = frame_power(x, win, hop, defect)
    res = segment(P, defect=defect, **kw)
    res['power'] = P
    res['samples'] = to_samples(res['segments'], hop, len(np.asarray(x).reshape(-1)))
    return res
