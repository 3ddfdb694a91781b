"""Every entry point of csrc/features.hip and csrc/ctc.hip called directly (ctypes, no Python wrapper), each against its float64
reference (tests/frontend_refs.py, itself pinned by tests/test_cpu_frontend_refs.py) under the derived per-element bound: the
assertion is ratio = max |got - ref| / bound <= 1 over ALL elements, never a max-normalised error.  Outputs start as NaN and are
followed by a guard region that is checked after every call; elements whose reference is inf or NaN must match exactly.

Which case reaches which kernel:

  kernel                       entry point               cases                       why
  logmel_kernel                w2l_logmel                LOGMEL_CASES[:6]            n_fft 64, 128, 256, 1024; win < n_fft; every n_mels, fb_range, noise, Tmax
  logmel512_kernel             w2l_logmel                LOGMEL_CASES[6:]            hop 160, 170: samples staged in LDS; 171, 200, 256: straight from memory
  feature_stats/apply_kernel   w2l_feature_normalize     NORM_CASES                  T_n 112 / 113 / 128 / 129: the 8-deep loop's first round; n_mels 80, 128: second grid row
  zero_rects_kernel            w2l_zero_rects            test_zero_rects             clipping, empty and out-of-range rectangles
  log_softmax_fwd/bwd_kernel   w2l_log_softmax_fwd/bwd   SOFTMAX_SHAPES              C > 64, CP == C, rows % 4 != 0, +-1e4, -inf
  argmax_kernel                w2l_argmax                test_argmax                 rows 1, 255, 257; NaN first / in the middle
  ctc_alpha_beta_kernel<..>    w2l_ctc_loss              ctc_tight_cases (34 kinds)  Smax at the edges of kWide and of the spt rounding, staged and not
                                                         ctc_full_case               every state slot of a thread live
  ctc_grad / ctc_loss_reduce   w2l_ctc_loss              ctc_sem_cases               blank, C, lengths 0 / clamped, infinities, N = 257
  (replay.hip)                 w2l_pad_vec_f32, w2l_fill_zero, w2l_add_i64_multi     one exact case each"""
import numpy as np
import pytest
import torch

import frontend_refs as R
from direct_helpers import GUARD, Buf, guards, last_error, p, ratio, record

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def L():
    from wav2letter_pytorch_amd import _lib
    assert torch.cuda.is_available()
    return _lib


def up(a, dtype=torch.float32):
    """a host array (or None) as a guarded device buffer"""
    return None if a is None else Buf(a.shape, dtype, torch.from_numpy(np.ascontiguousarray(a)))


def run(L, rc):
    """check the launch and wait for it; a HIP error ends the session: nothing more is launched on a device that has faulted"""
    try:
        L.check(rc)
        torch.cuda.synchronize()
    except Exception as e:                              # noqa: BLE001
        pytest.exit(f'HIP error in a direct front-end launch, nothing more is run: {e}', returncode=3)


def bounded(family, case, got, ref, bound):
    """non-finite reference elements equal, the rest within the bound; returns the ratio (recorded and printed)"""
    ok, g, r = R.split_nonfinite(got, ref)
    assert ok, f'{family} {case}: inf / NaN pattern differs from the reference'
    return record(family, case, ratio(g, r, np.where(np.isfinite(bound), bound, 0.0)))


# ---- w2l_logmel -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('c', R.LOGMEL_CASES, ids=lambda c: c.name)
def test_logmel(L, c):
    D = R.logmel_inputs(c)
    P, Pb, Lg, Lb = R.logmel_case_ref(c)
    audio, ns, noise = up(D['audio']), up(D['ns'], torch.int32), up(D['noise'])
    window, fbT, fr = up(D['window']), up(D['fbT']), up(D['fb_range'], torch.int32)
    Tmax = D['Tmax']
    frames = 1 + D['ns'] // c.hop
    assert (frames.max() < Tmax) == c.tmax_above and (c.tmax_above or frames.max() > Tmax)
    worst = 0.0
    for take_log, ref, bound in ((0, P, Pb), (1, Lg, Lb)):
        out = Buf((3, Tmax, c.n_mels))
        run(L, L.lib.w2l_logmel(p(L, audio), p(L, ns), p(L, noise), c.dither, R.PREEMPH, 3, D['stride'], p(L, window), c.win, c.n_fft,
                                c.hop, p(L, fbT), p(L, fr), c.n_mels, take_log, R.GUARD_LOG, p(L, out), Tmax, L.stream_ptr()))
        assert guards(audio, ns, noise, window, fbT, fr, out)
        got = out.np()
        for n in range(3):
            assert not got[n, min(frames[n], Tmax):].any(), 'frames past the utterance must be exactly 0'
        worst = max(worst, bounded('logmel512' if c.n_fft == 512 else 'logmel', f'{c.name}-log{take_log}', got, ref, bound))
    assert worst <= 1.0


def test_logmel_rejects_long_window(L):
    c = R.LOGMEL_CASES[0]
    D = R.logmel_inputs(c)
    audio, ns, window, fbT = up(D['audio']), up(D['ns'], torch.int32), up(R.hann(c.n_fft + 1)), up(D['fbT'])
    out = Buf((3, D['Tmax'], c.n_mels))
    rc = L.lib.w2l_logmel(p(L, audio), p(L, ns), None, 0.0, R.PREEMPH, 3, D['stride'], p(L, window), c.n_fft + 1, c.n_fft, c.hop,
                          p(L, fbT), None, c.n_mels, 1, R.GUARD_LOG, p(L, out), D['Tmax'], L.stream_ptr())
    torch.cuda.synchronize()
    assert rc != 0 and 'win_length' in last_error(L)
    assert torch.isnan(out.flat).all(), 'a rejected call writes nothing'


# ---- w2l_feature_normalize ----------------------------------------------------------------------------------------------------------

def normalize(L, x, ns, Tmax, n_mels):
    N = len(ns)
    xd, nsd = up(x), up(ns, torch.int32)
    mean, std, out = Buf((N, n_mels)), Buf((N, n_mels)), Buf((N, n_mels, Tmax))
    run(L, L.lib.w2l_feature_normalize(p(L, xd), p(L, nsd), R.NORM_HOP, N, Tmax, n_mels, R.NORM_EPS, p(L, mean), p(L, std), p(L, out),
                                       L.stream_ptr()))
    assert guards(xd, nsd, mean, std, out)
    return out.np(), mean.np(), std.np()


@pytest.mark.parametrize('n_mels,Tmax', R.NORM_CASES)
def test_feature_normalize(L, n_mels, Tmax):
    x, ns = R.normalize_inputs(n_mels, Tmax)
    out, outb, mean, meanb, std, stdb = R.feature_normalize_ref(x, ns, R.NORM_HOP, Tmax, R.NORM_EPS)
    g_out, g_mean, g_std = normalize(L, x, ns, Tmax, n_mels)
    case = f'm{n_mels}-T{Tmax}'
    for n, t in enumerate(R.NORM_TN):
        assert not g_out[n, :, min(t, Tmax):].any(), 'frames past the utterance must be exactly 0'
    one = R.NORM_TN.index(1)
    assert np.isnan(g_out[one, :, 0]).all() and np.isnan(g_std[one]).all(), 'T_n == 1 is NaN, as torch.std of one sample'
    r = [bounded('normalize', case + '-out', g_out, out, outb), bounded('normalize', case + '-mean', g_mean, mean, meanb),
         bounded('normalize', case + '-std', g_std, std, stdb)]
    assert max(r) <= 1.0


@pytest.mark.parametrize('n_mels,T_n', [(40, 16), (128, 128)])
def test_feature_normalize_constant(L, n_mels, T_n):
    """a power-of-two constant over a power-of-two count: the mean is exact, so is the zero"""
    Tmax = T_n + 5
    x = np.full((2, Tmax, n_mels), np.nan, dtype=np.float32)
    x[:, :T_n] = 0.5
    ns = np.array([(T_n - 1) * R.NORM_HOP, (T_n - 1) * R.NORM_HOP + 159], dtype=np.int32)
    g_out, g_mean, g_std = normalize(L, x, ns, Tmax, n_mels)
    assert not g_out.any() and (g_mean == 0.5).all() and (g_std == np.float32(R.NORM_EPS)).all()


# ---- w2l_zero_rects -----------------------------------------------------------------------------------------------------------------

def test_zero_rects(L):
    N, C, T = 3, 40, 70
    rng = np.random.default_rng(7)
    x = (1.0 + rng.random((N, C, T))).astype(np.float32)
    rects = np.array([[0, 3, 10, 5, 30], [0, 8, 14, 20, 40],            # overlapping
                      [1, 30, 55, 60, 90], [1, -4, 2, -7, 3],           # past C and T; negative starts
                      [2, 9, 9, 0, 70], [2, 12, 5, 0, 70], [2, 0, 40, 33, 33],      # f1 <= f0, t1 <= t0: empty
                      [3, 0, 40, 0, 70], [-1, 0, 40, 0, 70],            # n out of range
                      [2, 39, 40, 69, 70]], dtype=np.int32)
    want = x.copy()
    for n, f0, f1, t0, t1 in rects:
        if 0 <= n < N:
            want[n, max(f0, 0):max(f1, 0), max(t0, 0):max(t1, 0)] = 0.0
    xd, rd = up(x), up(rects, torch.int32)
    run(L, L.lib.w2l_zero_rects(p(L, xd), N, C, T, p(L, rd), len(rects), L.stream_ptr()))
    assert guards(xd, rd)
    assert np.array_equal(xd.np().view(np.uint32), want.view(np.uint32))
    assert (want == 0).sum() > 0 and want[2, 39, 69] == 0 and want[1, 0, 0] == 0
    xd = up(x)
    run(L, L.lib.w2l_zero_rects(p(L, xd), N, C, T, None, 0, L.stream_ptr()))          # R == 0 with a NULL list: nothing
    assert guards(xd) and np.array_equal(xd.np().view(np.uint32), x.view(np.uint32))
    record('zero_rects', 'exact', 0.0)


# ---- w2l_log_softmax_fwd / bwd ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('shape', R.SOFTMAX_SHAPES, ids=str)
@pytest.mark.parametrize('mode', [0, 1])
def test_log_softmax(L, shape, mode):
    N, T, C, CP = shape
    x, gout = R.softmax_inputs(shape)
    assert CP == C or np.isnan(x[:, C:]).all()                      # the junk columns must not be read into the result
    ref, rb = R.log_softmax_ref(x, C, mode)
    xd, out = up(x), Buf((N * T, C))
    run(L, L.lib.w2l_log_softmax_fwd(p(L, xd), N, T, C, CP, mode, p(L, out), L.stream_ptr()))
    assert guards(xd, out)
    r1 = bounded('softmax_fwd', f'{shape}-mode{mode}', out.np(), ref, rb)
    o32 = ref.astype(np.float32)
    gref, gb = R.log_softmax_bwd_ref(gout, o32, mode)
    gd, od, gl = up(gout), up(o32), Buf((N * T, C))
    run(L, L.lib.w2l_log_softmax_bwd(p(L, gd), p(L, od), N, T, C, mode, p(L, gl), L.stream_ptr()))
    assert guards(gd, od, gl)
    r2 = bounded('softmax_bwd', f'{shape}-mode{mode}', gl.np(), gref, gb)
    assert max(r1, r2) <= 1.0


# ---- w2l_argmax -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('rows', [1, 255, 257])
@pytest.mark.parametrize('C', [1, 29, 64])
def test_argmax(L, rows, C):
    rng = np.random.default_rng(rows * 100 + C)
    x = rng.integers(-3, 4, size=(rows, C)).astype(np.float32)      # small integers: ties in most rows
    for r in range(rows):
        k = r % 5
        if k == 1:
            x[r, C // 2] = np.nan                                    # a NaN in the middle (a larger value may follow)
            x[r, -1] = 100.0
        elif k == 2:
            x[r, 0] = np.nan                                         # a NaN first, another later
            x[r, -1] = np.nan
        elif k == 3:
            x[r] = -np.inf
        elif k == 4:
            x[r, :C // 2] = -np.inf
    xd, idx = up(x), Buf((rows,), torch.int32)
    run(L, L.lib.w2l_argmax(p(L, xd), rows, C, p(L, idx), L.stream_ptr()))
    assert guards(xd, idx)
    assert np.array_equal(idx.np(), R.argmax_ref(x))
    record('argmax', f'rows{rows}-C{C}', 0.0)


# ---- w2l_ctc_loss -----------------------------------------------------------------------------------------------------------------

def ctc_run(L, c):
    N, T, C = c.dims
    lp, tg = up(c.lp), up(c.targets, torch.int32)
    il, tl = up(c.in_len, torch.int32), up(c.tg_len, torch.int32)
    nll, loss = Buf((N,)), Buf((1,))
    grad = Buf((N, T, C)) if c.want_grad else None
    nbytes = L.lib.w2l_ctc_workspace_bytes(N, T, c.Smax)
    assert nbytes == 2 * N * T * (2 * c.Smax + 1) * 4
    ws = Buf((nbytes // 4,))
    run(L, L.lib.w2l_ctc_loss(p(L, lp), p(L, tg), p(L, il), p(L, tl), N, T, C, c.Smax, c.blank, c.zero_inf, p(L, nll), p(L, loss),
                              p(L, grad), p(L, ws), L.stream_ptr()))
    assert guards(lp, tg, il, tl, nll, loss, grad, ws), f'{c.name}: a guard region was written'
    return nll.np(), float(loss.np()[0]), None if grad is None else grad.np()


def ctc_check(L, c):
    r = R.ctc_case_ref(c)
    nll, loss, grad = ctc_run(L, c)
    fam = 'ctc_' + c.kind
    rs = [bounded(fam, c.name + '-nll', nll, r['nll'], r['nll_b']),
          bounded(fam, c.name + '-loss', np.array([loss]), np.array([r['loss']]), np.array([r['loss_b']]))]
    if grad is not None:
        for n in range(c.dims[0]):
            assert not grad[n, r['Tn'][n]:].any(), 'gradient rows past the input length must be exactly 0'
        spec = ~np.isnan(r['grad'])                     # an infinite utterance without zero_infinity: its gradient is not specified
        rs.append(bounded(fam, c.name + '-grad', grad[spec], r['grad'][spec], r['grad_b'][spec]))
    return max(rs)


@pytest.mark.parametrize('Smax,staged', R.ctc_tight_cases(), ids=lambda v: str(v))
def test_ctc_tight(L, Smax, staged):
    c = R.ctc_tight_case(Smax, staged)
    print('variant (NT, SPT, LP_LDS):', c.variant)
    assert ctc_check(L, c) <= 1.0


@pytest.mark.parametrize('Smax', R.FULL_SMAX)
def test_ctc_full_width(L, Smax):
    assert ctc_check(L, R.ctc_full_case(Smax)) <= 1.0


@pytest.mark.parametrize('c', R.ctc_sem_cases(), ids=lambda c: c.name)
def test_ctc_semantics(L, c):
    r = R.ctc_case_ref(c)
    assert bool(np.isinf(r['nll']).any()) == (c.infinite and not c.zero_inf)
    assert ctc_check(L, c) <= 1.0


# ---- what the engine calls every step (replay.hip) ------------------------------------------------------------------------------------

@pytest.mark.parametrize('n,cp', [(29, 64), (64, 64), (29, 128), (64, 128)])
@pytest.mark.parametrize('fill', [0.0, 1.0])
def test_pad_vec(L, n, cp, fill):
    src = np.random.default_rng(n + cp).standard_normal(n).astype(np.float32)
    sd, dst = up(src), Buf((cp,))
    run(L, L.lib.w2l_pad_vec_f32(p(L, sd), n, p(L, dst), cp, fill, L.stream_ptr()))
    assert guards(sd, dst)
    assert np.array_equal(dst.np(), np.concatenate([src, np.full(cp - n, fill, dtype=np.float32)]))


def test_fill_zero(L):
    b = Buf((1001,), torch.uint8)
    run(L, L.lib.w2l_fill_zero(p(L, b), 1001, L.stream_ptr()))
    assert guards(b) and not b.np().any()
    b = Buf((1001,), torch.uint8)
    run(L, L.lib.w2l_fill_zero(p(L, b), 999, L.stream_ptr()))
    assert guards(b) and not b.np()[:999].any() and (b.np()[999:] == 0xA5).all()


@pytest.mark.parametrize('n', [1, 70])
def test_add_i64_multi(L, n):
    start = (2 ** 32 - 5 + np.arange(n) * 3).astype(np.int64)
    if n > 1:
        start[-1] = -9
    cells = torch.full((n + GUARD,), 0x5A5A5A5A5A5A, dtype=torch.int64, device='cuda')
    cells[:n] = torch.from_numpy(start)
    table = torch.tensor([cells.data_ptr() + 8 * i for i in range(n)], dtype=torch.int64, device='cuda')
    for delta in (7, 2 ** 33 + 1):                       # across 2^32 in the low word, and a delta wider than 32 bits
        run(L, L.lib.w2l_add_i64_multi(L.ptr(table), n, delta, L.stream_ptr()))
        start = start + delta
        assert np.array_equal(cells[:n].cpu().numpy(), start) and bool((cells[n:] == 0x5A5A5A5A5A5A).all())
