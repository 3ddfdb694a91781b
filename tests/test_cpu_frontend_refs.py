"""The float64 references of tests/frontend_refs.py pinned (no GPU): log-mel against torch.stft in float64, the normalisation against
torch.std, the softmax pair against torch float64 autograd, CTC against F.ctc_loss on float64 tensors -- and the bounds shown to
have teeth: every planted defect, applied to the reference as a model of a kernel fault, exceeds its bound on a case the GPU
tests run.  The conditions the GPU tests lean on are asserted for every shared case: all 34 CTC kernel variants reached, no zero
bound under a non-zero reference, no infinite bound outside the cases built for infinities, tight CTC bounds tight."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import frontend_refs as R
from direct_helpers import ratio


def caught(got, ref, bound):
    """a defective result is caught if its non-finite pattern differs or its ratio exceeds 1"""
    ok, g, r = R.split_nonfinite(got, ref)
    return (not ok) or ratio(g, r, np.where(np.isfinite(bound), bound, 0.0)) > 1.0


# ---- references against torch float64 ----------------------------------------------------------------------------------------

@pytest.mark.parametrize('c', R.LOGMEL_CASES, ids=lambda c: c.name)
def test_logmel_ref_against_torch_stft(c):
    D = R.logmel_inputs(c)
    P, Pb, Lg, Lb = R.logmel_case_ref(c)
    win = torch.from_numpy(D['window']).double()
    fb = torch.from_numpy(D['fbT']).double()
    for n, L in enumerate(D['ns']):
        x = torch.from_numpy(D['audio'][n, :L]).double()
        if D['noise'] is not None:
            x = x + torch.from_numpy(D['noise'][n, :L]).double() * float(np.float32(c.dither))
        x = torch.cat([x[:1], x[1:] - float(np.float32(R.PREEMPH)) * x[:-1]])
        S = torch.stft(x, c.n_fft, c.hop, c.win, win, center=True, pad_mode='reflect', return_complex=True)     # [bins][frames]
        mel = (S.abs() ** 2).T @ fb
        frames = mel.shape[0]
        assert frames == 1 + L // c.hop
        live = min(frames, D['Tmax'])
        scale = float(mel.max())
        assert np.abs(P[n, :live] - mel[:live].numpy()).max() <= 1e-12 * scale
        assert np.abs(Lg[n, :live] - torch.log1p(mel[:live] + R.GUARD_LOG).numpy()).max() <= 1e-12 * (1 + np.log1p(scale))
        assert not P[n, live:].any() and not Lg[n, live:].any() and not Pb[n, live:].any() and not Lb[n, live:].any()
    assert (Pb[P != 0] > 0).all() and (Lb[Lg != 0] > 0).all() and np.isfinite(Pb).all() and np.isfinite(Lb).all()


@pytest.mark.parametrize('n_mels,Tmax', R.NORM_CASES)
def test_normalize_ref_against_torch_std(n_mels, Tmax):
    x, ns = R.normalize_inputs(n_mels, Tmax)
    out, outb, mean, meanb, std, stdb = R.feature_normalize_ref(x, ns, R.NORM_HOP, Tmax, R.NORM_EPS)
    eps = float(np.float32(R.NORM_EPS))
    for n, t in enumerate(R.NORM_TN):
        T_n = min(t, Tmax)
        assert T_n == min(1 + ns[n] // R.NORM_HOP, Tmax)
        xt = torch.from_numpy(x[n, :T_n]).double()
        assert np.abs(mean[n] - xt.mean(0).numpy()).max() <= 1e-12
        assert not out[n, :, T_n:].any() and not outb[n, :, T_n:].any()
        if T_n == 1:
            assert np.isnan(std[n]).all() and np.isnan(out[n, :, 0]).all()
            continue
        s = xt.std(0) + eps
        assert np.abs(std[n] - s.numpy()).max() <= 1e-12
        assert np.abs(out[n, :, :T_n] - ((xt - xt.mean(0)) / s).T.numpy()).max() <= 1e-11
        assert (outb[n, :, :T_n] > 0).all() and np.isfinite(outb[n]).all() and (stdb[n] > 0).all() and (meanb[n] > 0).all()
        # the bound is a bound of fp32 arithmetic, not a loose one: relative to the unit-variance output it stays near 1e-5
        assert outb[n].max() < 2e-4


@pytest.mark.parametrize('shape', R.SOFTMAX_SHAPES, ids=str)
@pytest.mark.parametrize('mode', [0, 1])
def test_softmax_refs_against_torch(shape, mode):
    N, T, C, CP = shape
    x, gout = R.softmax_inputs(shape)
    out, ob = R.log_softmax_ref(x, C, mode)
    xt = torch.from_numpy(x[:, :C]).double().requires_grad_(True)
    want = F.log_softmax(xt, dim=1) if mode == 0 else F.softmax(xt, dim=1)
    ok, g, r = R.split_nonfinite(want.detach().numpy(), out)
    assert ok and np.abs(g - r).max() <= 1e-12 * max(1.0, np.abs(r).max())
    fin = np.isfinite(out)
    assert (ob[fin & (out != 0)] > 0).all() and np.isfinite(ob[fin]).all()
    big = np.isfinite(x[:, :C]).all(axis=1) & (np.abs(x[:, :C]).max(axis=1) > 5e3)
    assert big.any() == (N * T > 1) and np.isfinite(out[big]).all()          # logits near +-1e4 stay finite
    # backward on the rows torch can differentiate (all entries finite): the device is handed the fp32 out
    rows = np.isfinite(x[:, :C]).all(axis=1)
    o32 = out.astype(np.float32)
    gl, gb = R.log_softmax_bwd_ref(gout, o32, mode)
    xr = torch.from_numpy(x[rows][:, :C]).double().requires_grad_(True)
    y = F.log_softmax(xr, dim=1) if mode == 0 else F.softmax(xr, dim=1)
    y.backward(torch.from_numpy(gout[rows]).double())
    exact, _ = R.log_softmax_bwd_ref(gout[rows], y.detach().numpy(), mode)
    assert np.abs(exact - xr.grad.numpy()).max() <= 1e-12 * max(1.0, np.abs(exact).max())
    assert np.isfinite(gb[rows]).all() and (gb[rows][gl[rows] != 0] > 0).all()


def all_ctc_cases():
    return ([R.ctc_tight_case(*k) for k in R.ctc_tight_cases()] + [R.ctc_full_case(S) for S in R.FULL_SMAX] + list(R.ctc_sem_cases()))


def torch_ctc(c, S, Tn):
    """F.ctc_loss on float64 CPU tensors with the CLAMPED lengths, utterances with Tn > 0 only (torch rejects the others);
    the header's loss and gradient are formed from the per-utterance values"""
    N, T, Cc = c.dims
    keep = np.nonzero(Tn > 0)[0]
    lp = torch.from_numpy(c.lp[keep]).double().requires_grad_(True)
    nll = F.ctc_loss(lp.transpose(0, 1), torch.from_numpy(c.targets[keep].astype(np.int64)), torch.from_numpy(Tn[keep]),
                     torch.from_numpy(S[keep]), blank=c.blank, reduction='none', zero_infinity=bool(c.zero_inf))
    w = 1.0 / (N * np.maximum(S[keep], 1))
    fin = torch.isfinite(nll)
    (nll[fin] * torch.from_numpy(w)[fin]).sum().backward()
    return keep, nll.detach().numpy(), lp.grad.numpy()


@pytest.mark.parametrize('c', all_ctc_cases(), ids=lambda c: c.name)
def test_ctc_ref_against_torch(c):
    r = R.ctc_case_ref(c)
    S, Tn = r['S'], r['Tn']
    N, T, Cc = c.dims
    keep, nll, grad = torch_ctc(c, S, Tn)
    tol = 1e-12 * max(1.0, float(np.abs(nll[np.isfinite(nll)]).max(initial=0.0)))
    assert np.array_equal(np.isinf(r['nll'][keep]), np.isinf(nll))
    fin = np.isfinite(nll)
    assert np.abs(r['nll'][keep][fin] - nll[fin]).max(initial=0.0) <= tol
    if c.want_grad:
        for i, n in enumerate(keep):
            if np.isinf(r['nll'][n]):
                # torch gives NaN here without zero_infinity; the header specifies nothing, the reference marks it NaN: not asserted
                assert np.isnan(r['grad'][n]).all()
                continue
            # torch's backward gives NaN where a log-probability is -inf (inf - inf); the header's (exp(lp) - posterior) is 0 there
            at_inf = np.isinf(c.lp[n])
            assert not r['grad'][n][at_inf].any()
            assert np.abs(r['grad'][n] - grad[i])[~at_inf].max() <= 1e-12
            assert not r['grad'][n, Tn[n]:].any()
    # what torch does not accept, as the header states it: clamped lengths (above); Tn == 0 -> nll 0 if S == 0, else 0 / inf
    for n in np.nonzero(Tn == 0)[0]:
        want = 0.0 if (S[n] == 0 or c.zero_inf) else np.inf
        assert r['nll'][n] == want and not r['grad'][n].any()
    want = (r['nll'] / np.maximum(S, 1)).sum() / N
    assert r['loss'] == want or abs(r['loss'] - want) <= 1e-12 * abs(want)
    assert np.isinf(r['loss']) == bool(np.isinf(r['nll']).any())


# ---- conditions of the shared cases --------------------------------------------------------------------------------------------

def test_ctc_variant_coverage():
    want = {(nt, 1, s) for nt in R.KWIDE for s in (True, False)} | {(1024, k, s) for k in (2, 3, 4, 6, 8) for s in (True, False)}
    assert len(want) == 34
    got = {R.ctc_tight_case(*k).variant for k in R.ctc_tight_cases()}
    assert got == want
    assert {R.ctc_full_case(S).variant[:2] for S in R.FULL_SMAX} == {(1024, k) for k in (1, 2, 3, 4, 6, 8)}
    # the restated dispatch at the edges of kWide and of the spt rounding
    assert [R.ctc_variant(s, 48, 29)[:2] for s in (31, 32, 511, 512, 1023, 1024, 2047, 2048, 2559, 2560, 3071, 3072, 4095)] == [
        (64, 1), (128, 1), (1024, 1), (1024, 2), (1024, 2), (1024, 3), (1024, 4), (1024, 6), (1024, 6), (1024, 6), (1024, 6),
        (1024, 8), (1024, 8)]
    # staging: 150 KB less the two state buffers
    assert R.ctc_variant(31, 1319, 29)[2] and not R.ctc_variant(31, 1320, 29)[2]
    assert R.ctc_variant(4095, 758, 29)[2] and not R.ctc_variant(4095, 759, 29)[2]


@pytest.mark.parametrize('c', all_ctc_cases(), ids=lambda c: c.name)
def test_ctc_case_conditions(c):
    r = R.ctc_case_ref(c)
    g, gb = r['grad'], r['grad_b']
    ok = np.isfinite(g)
    assert (gb[ok & (g != 0)] > 0).all()
    fin = np.isfinite(r['nll'])
    assert (r['nll_b'][fin & (r['nll'] != 0)] > 0).all()
    if not c.infinite:
        assert np.isfinite(gb).all() and np.isfinite(r['nll_b']).all() and np.isfinite(r['loss_b']) and fin.all()
    if c.kind == 'tight':
        nz = ok & (g != 0)
        assert nz.sum() > 1000
        assert (gb[nz] < 1e-3 * np.abs(g[nz])).mean() >= 0.95
        assert (r['nll_b'] < 1e-4 * np.abs(r['nll'])).all()


# ---- planted defects -------------------------------------------------------------------------------------------------------------

LOGMEL_DEFECTS = ['reflect_edge', 'woff0', 'preemph_wrap', 'twiddle_sign', 'no_nyquist', 'filter_short', 'log_not_log1p',
                  'frames_L_over_hop', 'last_frame_zero']


@pytest.mark.parametrize('defect', LOGMEL_DEFECTS)
def test_logmel_defect_exceeds_bound(defect):
    hits = []
    for c in R.LOGMEL_CASES:
        P, Pb, Lg, Lb = R.logmel_case_ref(c)
        dP, _, dL, _ = R.logmel_case_ref(c, defect)
        if caught(dP, P, Pb) or caught(dL, Lg, Lb):
            hits.append(c.name)
    assert hits, defect
    print(defect, len(hits), 'of', len(R.LOGMEL_CASES))


@pytest.mark.parametrize('defect', ['biased', 'eps_under_root', 'stats_over_Tmax', 'tail_skip', 'no_transpose_m64'])
def test_normalize_defect_exceeds_bound(defect):
    hits = 0
    for n_mels, Tmax in R.NORM_CASES:
        x, ns = R.normalize_inputs(n_mels, Tmax)
        out, outb, mean, meanb, std, stdb = R.feature_normalize_ref(x, ns, R.NORM_HOP, Tmax, R.NORM_EPS)
        d = R.feature_normalize_ref(x, ns, R.NORM_HOP, Tmax, R.NORM_EPS, defect)
        hits += caught(d[0], out, outb) or caught(d[2], mean, meanb) or caught(d[4], std, stdb)
    assert hits, defect


@pytest.mark.parametrize('defect,mode', [('max_over_CP', 0), ('skip_ge64', 0), ('skip_ge64', 1)])
def test_softmax_defect_exceeds_bound(defect, mode):
    hits = 0
    for shape in R.SOFTMAX_SHAPES:
        x, _ = R.softmax_inputs(shape)
        out, ob = R.log_softmax_ref(x, shape[2], mode)
        hits += caught(R.log_softmax_ref(x, shape[2], mode, defect)[0], out, ob)
    assert hits, defect


def test_softmax_bwd_defect_exceeds_bound():
    hits = 0
    for shape in R.SOFTMAX_SHAPES:
        x, gout = R.softmax_inputs(shape)
        o32 = R.log_softmax_ref(x, shape[2], 1)[0].astype(np.float32)
        gl, gb = R.log_softmax_bwd_ref(gout, o32, 1)
        hits += caught(R.log_softmax_bwd_ref(gout, o32, 1, 'bwd_sum_g')[0], gl, gb)
    assert hits


CTC_DEFECTS = ['skip_equal', 'no_skip3', 'beta_T', 'lse2_last_only', 'slot_ge_nt', 'gs_noS', 'rows_beyond', 'blank0']


def ctc_caught(c, defect):
    r = R.ctc_case_ref(c)
    if caught(R.ctc_case_ref(c, defect, want_grad=False)['nll'], r['nll'], r['nll_b']):
        return True
    if not c.want_grad:
        return False
    d = R.ctc_case_ref(c, defect)
    m = ~np.isnan(r['grad'])                        # an unspecified gradient is not compared
    return caught(d['grad'][m], r['grad'][m], r['grad_b'][m])


@pytest.mark.parametrize('defect', CTC_DEFECTS)
def test_ctc_defect_exceeds_bound(defect):
    if defect == 'slot_ge_nt':                      # the wide bound of the full-width cases still sees it, in every SPT > 1 kernel
        cases = [R.ctc_full_case(S) for S in R.FULL_SMAX if R.ctc_variant(S, 1, 1)[1] > 1]
        assert len(cases) == 5 and all(ctc_caught(c, defect) for c in cases)
        return
    cases = [R.ctc_tight_case(*k) for k in R.ctc_tight_cases()[:4]] + list(R.ctc_sem_cases())
    hits = [c.name for c in cases if ctc_caught(c, defect)]
    assert hits, defect
    print(defect, hits)
