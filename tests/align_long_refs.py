"""What tests/test_cpu_align_long.py and tests/test_gpu_align_long.py share: the inputs of the device cases, and ``tiled_align``,
a NumPy emulation of csrc/ctc_align_long.hip's scheme in float32 -- time blocks, state tiles with a halo below, owned-only
stores of the column and of the packed move words, two columns swapped per block, the windowed back-trace -- with the defects
the CPU tests plant in it.  The emulation is not the reference: alignment.viterbi_align_host is, for both."""
import numpy as np

from wav2letter_pytorch_amd.alignment import HostAlignment

DEFECTS = ('short_halo', 'halo_moves_stored', 'no_swap', 'short_window', 'no_flush')
GARBAGE = np.uint32(0xAAAAAAAA)            # what the move words hold before a store: every move "from s-2"


def log_probs(rng, t, a, holes=0.0):
    """float32 log-softmax of random logits [t, a], a share of ``holes`` entries at -inf"""
    z = rng.standard_normal((t, a)) * 2.0
    z -= z.max(-1, keepdims=True)
    lp = (z - np.log(np.exp(z).sum(-1, keepdims=True))).astype(np.float32)
    if holes:
        lp[rng.random(lp.shape) < holes] = -np.inf
    return lp


def target(rng, a, s, blank=0, p_repeat=0.3):
    """s random labels with runs of repeats (p_repeat = 0: none)"""
    row = []
    while len(row) < s:
        if row and rng.random() < p_repeat:
            row.append(row[-1])
        else:
            c = int(rng.integers(0, a - 1))
            c += c >= blank
            if p_repeat == 0 and row and c == row[-1]:
                continue
            row.append(c)
    return row


def needed(row):
    return len(row) + sum(x == y for x, y in zip(row, row[1:]))


def grid_cases():
    """T in {1, 2, 16, 17, 70} x S in {0, 1, 31, 32, 33, 100}, with runs of repeats; where T is too short the answer is
    'no path'.  T = 70, S = 100 under (16, 64): five time blocks by four tiles."""
    out = []
    for t in (1, 2, 16, 17, 70):
        for s in (0, 1, 31, 32, 33, 100):
            rng = np.random.default_rng(1000 * t + s)
            out.append(('grid T=%d S=%d' % (t, s), log_probs(rng, t, 29, holes=0.05 if t == 70 else 0.0), target(rng, 29, s, p_repeat=0.2)))
    return out


def single_path_cases():
    """T = S + repeats exactly; T = S without repeats (the path climbs two states every frame: the one input that needs the
    whole halo); and each with one frame fewer (no path)"""
    out = []
    rng = np.random.default_rng(77)
    row = target(rng, 29, 80, p_repeat=0.4)
    lp = log_probs(rng, needed(row), 29)
    out += [('single T=S+repeats', lp, row), ('single T=S+repeats-1', lp[:-1], row)]
    row = target(rng, 29, 100, p_repeat=0.0)
    lp = log_probs(rng, 100, 29)
    out += [('single T=S', lp, row), ('single T=S-1', lp[:-1], row)]
    # The T = S staircase at an odd offset from the tiles.  Tiles start at multiples of 64 and time blocks at multiples of 16,
    # so the plain staircase (state 2 t + 1 at frame t) never runs from just below a window to the first owned label state.
    # Held back 31 frames on its first label (every other emission of a frame at -inf: still one path), it is at state 1 at
    # frame 31 and at state 65 at frame 63: under (32, 64) from two states below tile 1's 64-state halo to its second own state.
    lp = np.full((131, 29), -np.inf, dtype=np.float32)
    forced = [row[0]] * 31 + row
    lp[np.arange(131), forced] = log_probs(rng, 131, 29)[np.arange(131), forced]
    out.append(('single staircase+31', lp, row))
    return out


SMALL_PLANS = [(16, 64), (48, 2048)]       # the forced plan, and a second with another tb and the widest tile
SINGLE_PLANS = [(16, 64), (32, 64), (32, 128), (48, 2048)]      # (32, 64), (32, 128): the halo is exactly 2 tb states


def window(tb, sb):
    """(threads, states per thread) of a forward workgroup, as long_plan of ctc_align_long.hip sets them"""
    w = sb + 2 * tb
    spt = 1 if w <= 1024 else (2 if w <= 2048 else 4)
    return -(-w // (64 * spt)) * 64, spt


def tiled_align(lp, tg, blank, tb, sb, halo=None, defect=None):
    """the tiled scheme on the host; ``halo``: states below a tile's own that its workgroup carries (default: the kernel's,
    threads x states per thread - sb >= 2 tb); ``defect``: one of DEFECTS"""
    assert defect is None or defect in DEFECTS
    f32 = np.float32
    lp = np.asarray(lp, dtype=f32)
    t_n, a = lp.shape
    tg = np.asarray(tg, dtype=np.int64).reshape(-1)
    s_n = tg.size
    n_st = 2 * s_n + 1
    tiles = -(-n_st // sb)
    lpad = tiles * sb
    if halo is None:
        nt, spt = window(tb, sb)
        halo = nt * spt - sb
    if defect == 'short_halo':
        halo = 2 * tb - 2
    ninf = f32(-np.inf)
    ext = np.full(lpad, blank, dtype=np.int64)
    ext[1:n_st:2] = tg
    skip = np.zeros(lpad, dtype=bool)
    if s_n > 1:
        skip[3:n_st:2] = tg[1:] != tg[:-1]
    cols = [np.full(lpad, ninf, dtype=f32), np.full(lpad, ninf, dtype=f32)]
    cols[0][:min(2, n_st)] = lp[0, ext[:min(2, n_st)]]
    chunks = (t_n + 15) >> 4
    words = np.full((chunks, lpad), GARBAGE, dtype=np.uint32)
    flip = 0
    blocks = -(-t_n // tb)
    with np.errstate(invalid='ignore'):
        for b in range(blocks):
            t0, t1 = max(b * tb, 1), min((b + 1) * tb, t_n)
            if t0 >= t1:
                continue
            cin, cout = cols[flip], cols[flip ^ 1]
            for i in range(tiles):
                own0 = i * sb
                base = own0 - halo
                top = own0 + sb
                lo = max(base, 0)                                  # cells below state 0 hold -inf and stay there
                pad = lo - base
                n = halo + sb
                cur = np.full(n, ninf, dtype=f32)
                cur[pad:] = cin[lo:top]
                w_ext = np.full(n, blank, dtype=np.int64)
                w_ext[pad:] = ext[lo:top]
                w_skip = np.zeros(n, dtype=bool)
                w_skip[pad:] = skip[lo:top]
                dead = np.arange(base, top) >= n_st
                bw = np.zeros(n, dtype=np.uint32)
                for t in range(t0, t1):
                    a1 = np.concatenate(([ninf], cur[:-1]))        # the guards below the window
                    a2 = np.concatenate(([ninf, ninf], cur[:-2]))
                    a2[~w_skip] = ninf
                    best = cur.copy()
                    mv = np.zeros(n, dtype=np.uint32)
                    m = a1 > best
                    best[m] = a1[m]
                    mv[m] = 1
                    m = a2 > best
                    best[m] = a2[m]
                    mv[m] = 2
                    new = best + lp[t, w_ext]
                    new[best == ninf] = ninf
                    new[dead] = ninf
                    cur = new
                    bw |= mv << np.uint32(2 * (t & 15))
                    if (t & 15) == 15 or (t == t1 - 1 and defect != 'no_flush'):
                        if defect == 'halo_moves_stored':
                            words[t >> 4, lo:top] = bw[pad:]
                        else:
                            words[t >> 4, own0:top] = bw[halo:]
                        bw[:] = 0
                cout[own0:top] = cur[halo:]
            if defect != 'no_swap':
                flip ^= 1
    col = cols[flip]
    end = n_st - 1
    if n_st > 1 and col[n_st - 2] >= col[n_st - 1]:
        end = n_st - 2
    best = col[end]
    if not best > ninf:
        none = np.full(s_n, -1, dtype=np.int32)
        return HostAlignment(f32(-np.inf), np.full(t_n, -1, dtype=np.int32), none, none.copy(), False)
    # the back-trace: per time block the words of the 2 tb - 1 states at and below the entry state, walked in that window
    w_n = 2 * tb - 1 - (defect == 'short_window')
    states = np.empty(t_n, dtype=np.int64)
    s = end
    for b in range(blocks - 1, -1, -1):
        t_lo, t_hi = max(b * tb, 1), min((b + 1) * tb, t_n) - 1
        if t_lo > t_hi:
            continue
        c0 = (b * tb) >> 4
        nc = (t_hi >> 4) - c0 + 1
        wbase = s - (w_n - 1)
        win = np.zeros((nc, w_n), dtype=np.uint32)
        lo = max(wbase, 0)
        win[:, lo - wbase:] = words[c0:c0 + nc, lo:s + 1]
        for t in range(t_hi, t_lo - 1, -1):
            states[t] = s
            j = s - wbase
            word = win[(t >> 4) - c0, j] if 0 <= j < w_n else np.uint32(0)
            s -= int((word >> np.uint32(2 * (t & 15))) & np.uint32(3))
            s = max(s, 0)
    states[0] = s
    full_ext = ext[:n_st]
    path = full_ext[states].astype(np.int32)
    starts = np.full(s_n, -1, dtype=np.int32)
    ends = np.full(s_n, -1, dtype=np.int32)
    own = (states & 1) == 1
    first = own & np.concatenate(([True], states[1:] != states[:-1]))
    last = own & np.concatenate((states[1:] != states[:-1], [True]))
    starts[states[first] >> 1] = np.nonzero(first)[0]
    ends[states[last] >> 1] = np.nonzero(last)[0]
    return HostAlignment(best, path, starts, ends, True)


def same(x, y):
    """two HostAlignments (or an Alignment row as a HostAlignment): the score's bytes, path, starts, ends and feasibility"""
    return (bool(x.feasible) == bool(y.feasible) and np.float32(x.score).tobytes() == np.float32(y.score).tobytes()
            and np.array_equal(x.path, y.path) and np.array_equal(x.starts, y.starts) and np.array_equal(x.ends, y.ends))
