"""Crafted power arrays for the decision pass of the segmentation rule, with answers derived by hand (in the comments), shared
by tests/test_cpu_vad.py (the numpy reference must give them) and tests/test_gpu_vad.py (the kernel must).  Absolute mode:
thr_on = 1.0, thr_off = 0.5.  H = 2.0 is speech, L = 0.25 is silence, M = 0.75 lies between the thresholds ("keep")."""
import numpy as np

H, M, L = 2.0, 0.75, 0.25
THR = dict(thr_on=1.0, thr_off=0.5)


def arr(*parts):
    """(value, count) pairs or bare values -> float32 array"""
    out = []
    for p in parts:
        if isinstance(p, tuple):
            out += [p[0]] * p[1]
        else:
            out.append(p)
    return np.asarray(out, dtype=np.float32)


def case(P, segments, min_silence=1, min_speech=1, pad=0, max_frames=100000, **kw):
    kw = dict(THR, **kw)
    return dict(P=P, want=np.asarray(segments, dtype=np.int64).reshape(-1, 2),
                kw=dict(min_silence=min_silence, min_speech=min_speech, pad=pad, max_frames=max_frames, **kw))


CASES = {
    # f:   0     1    2    3    4     5     6     7    8    9
    # P: 0.25  1.0  0.5  0.5  0.25  0.75  0.75  1.0  0.5  0.25
    # s:   0     1    1    1    0     0     0     1    1    0      1.0 >= thr_on switches on; 0.5 is not < thr_off: keep
    'ties': case(arr(L, 1.0, 0.5, 0.5, L, M, M, 1.0, 0.5, L), [[1, 4], [7, 9]]),
    # runs [0,2) [4,6) [9,11): the gap 4 - 2 = 2 = min_silence - 1 closes, the gap 9 - 6 = 3 = min_silence stays
    'gap': case(arr((H, 2), (L, 2), (H, 2), (L, 3), (H, 2)), [[0, 6], [9, 11]], min_silence=3),
    # runs [0,1) [2,3) [5,6) [10,11): gaps 1, 2 close one after the other (a chain of three), the gap 4 stays
    'chain': case(arr(H, L, H, L, L, H, (L, 4), H), [[0, 6], [10, 11]], min_silence=3),
    # runs [0,2) of min_speech - 1 = 2 frames (dropped) and [6,9) of min_speech = 3 frames (kept)
    'short': case(arr((H, 2), (L, 4), (H, 3), L), [[6, 9]], min_speech=3),
    # runs [0,1) [2,3): closing first joins them into [0,3), 3 frames = min_speech, kept.  (Dropping first would leave nothing.)
    'close_then_drop': case(arr(H, L, H, (L, 4)), [[0, 3]], min_silence=3, min_speech=3),
    # F = 14, runs [1,3) [12,14), pad 3: [1-3, 3+3) clips to [0,6); [12-3, 14+3) clips to [9,14); 9 > 6: no merge
    'pad_clip': case(arr(L, (H, 2), (L, 9), (H, 2)), [[0, 6], [9, 14]], pad=3),
    # F = 14, runs [2,4) [8,10), pad 2: [0,6) and [6,12) touch -> one run [0,12)
    'pad_merge': case(arr((L, 2), (H, 2), (L, 4), (H, 2), (L, 4)), [[0, 12]], pad=2),
    # runs [2,4) [9,11), pad 2: [0,6) and [7,13) do not touch
    'pad_apart': case(arr((L, 2), (H, 2), (L, 5), (H, 2), (L, 3)), [[0, 6], [7, 13]], pad=2),
    # max_frames 8, h = 4.  [0,8): 8 frames = max_frames, whole.  [10,19): 9 frames: window [14, min(18, 15)) = {14}: cut at 14;
    # [14,19) has 5 frames
    'split_edge': case(arr((H, 8), (L, 2), (H, 9)), [[0, 8], [10, 14], [14, 19]], max_frames=8),
    # max_frames 8, h = 4, run [0,14) (every power >= thr_on): window [4, min(8, 10)) = [4,8) holds 3 2 2 3: the minimum 2 lies
    # at 5 and 6, the lowest index wins: cut at 5.  [5,14) has 9 frames: window [9, min(13, 10)) = {9}: cut at 9.  [9,14): 5 frames
    'split_ties': case(arr((5.0, 4), 3.0, 2.0, 2.0, 3.0, (5.0, 6)), [[0, 5], [5, 9], [9, 14]], max_frames=8),
    'one_on': case(arr(H), [[0, 1]]),
    'one_off': case(arr(L), []),
    'zeros': case(arr((0.0, 50)), []),
    # on at 0, then 3000 frames of "keep": the state must cross every 1024-frame tile: [0,3001).  Off at 3001, 3000 frames of
    # "keep" stay off.  On at 6002, off at 6003
    'carry': case(arr(H, (M, 3000), L, (M, 3000), H, L), [[0, 3001], [6002, 6003]]),
    # 1000 equal silence powers and 7 speech frames at 500..506
    'duplicates': case(arr((L, 500), (H, 7), (L, 500)), [[500, 507]]),
}

# adaptive mode, by hand: sorted P = 0.25 x 1000, 2.0 x 7; q = 0.05: k = floor(0.05 * 1006) = 50 -> floor 0.25, peak 2.0;
# thr_on = max(1e-10, min(0.25 * 10, sqrt(0.25 * 2.0) = 0.70710678...)) = sqrt(0.5); thr_off = thr_on / 2
ADAPTIVE = dict(P=CASES['duplicates']['P'], want=np.asarray([[500, 507]], dtype=np.int64), floor=0.25, peak=2.0, thr_on=0.5 ** 0.5,
                thr_off=0.5 ** 0.5 / 2,
                kw=dict(q=0.05, r_on=10.0, r_hyst=0.5, abs_min=1e-10, min_silence=1, min_speech=1, pad=0, max_frames=100000))


def synthetic_recording(seed=0, noise_dbfs=-60.0, rate=16000, hop=160):
    """30 s: Gaussian noise at ``noise_dbfs`` plus 440 Hz tone bursts of amplitude 0.5 whose edges lie on frame boundaries:
    [1.0, 3.0) and [3.2, 4.0) s (the 0.2 s gap between them must be closed), [5.0, 5.05) s (50 ms: must be dropped) and
    [6.0, 25.0) s (19 s: must take a forced cut at max_seconds = 15), which has a 0.1 s dip at [16.0, 16.1) s: ten hops whose
    power falls by 4 per hop to 1 / 1024 of the burst's over two equal hops in the middle and rises again, so the frame over
    those two hops is the minimum of its neighbourhood by a factor of 2.5."""
    rng = np.random.default_rng(seed)
    n = 30 * rate
    x = (10.0 ** (noise_dbfs / 20.0)) * rng.standard_normal(n)
    t = np.arange(n) / rate
    gain = np.zeros(n)
    for a, b in ((1.0, 3.0), (3.2, 4.0), (5.0, 5.05), (6.0, 25.0)):
        gain[int(round(a * rate)): int(round(b * rate))] = 1.0
    d0 = 16 * rate
    for j, e in enumerate((1, 2, 3, 4, 5, 5, 4, 3, 2, 1)):           # power 4^-e  =  amplitude 2^-e
        gain[d0 + j * hop: d0 + (j + 1) * hop] = 2.0 ** -e
    return (x + 0.5 * gain * np.sin(2 * np.pi * 440.0 * t)).astype(np.float32)


def random_cases(seed=0):
    """power arrays of the frame counts at which the kernel's tiling changes (1, 63, 64, 65, 1025, 5 * 1024 + 37), drawn from few
    distinct values (many duplicates, ties at both thresholds), with parameters that make every step of the rule act"""
    rng = np.random.default_rng(seed)
    values = np.asarray([0.0, 0.25, 0.5, 0.75, 1.0, 2.0, 3.0], dtype=np.float32)
    out = {}
    for F in (1, 63, 64, 65, 1025, 5 * 1024 + 37):
        # a slowly changing level plus jitter: runs and gaps of many lengths
        level = np.repeat(rng.integers(0, len(values), size=F // 7 + 1), 7)[:F]
        jitter = rng.integers(-1, 2, size=F) * (rng.random(F) < 0.3)
        P = values[np.clip(level + jitter, 0, len(values) - 1)]
        out[f'random_{F}'] = dict(P=P, kw=dict(THR, min_silence=3, min_speech=4, pad=2, max_frames=24))
    return out
