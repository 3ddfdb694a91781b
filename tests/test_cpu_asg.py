"""ASG criterion, host side: the repetition encoding, the float64 references the GPU tests compare against (pinned here by
brute-force enumeration of every frame path), and the configuration key ``model.criterion``."""
import numpy as np
import pytest
import torch

import asg_refs as R
from direct_helpers import ratio

LETTERS = {c: i + 1 for i, c in enumerate('abcdefghijklmnopqrstuvwxyz')}      # 0 is the repeat label


def _ids(s):
    return [LETTERS[c] for c in s]


@pytest.mark.parametrize('word,encoded', [('hello', 'hel_o'), ('aaa', 'a_a'), ('aaaa', 'a_a_'), ('a', 'a'), ('', ''),
                                          ('abba', 'ab_a'), ('lll', 'l_l')])
def test_encode_decode_round_trip(word, encoded):
    from wav2letter_pytorch_amd.asg import decode_repeats, encode_repeats
    enc = encode_repeats(_ids(word))
    assert enc == [0 if c == '_' else LETTERS[c] for c in encoded]
    assert len(enc) == len(word) and all(a != b for a, b in zip(enc, enc[1:]))
    assert decode_repeats(enc) == _ids(word)
    assert enc == R.encode(_ids(word))                 # the references' own encoder agrees


def test_decode_of_collapsed_frame_paths():
    from wav2letter_pytorch_amd.asg import collapse_frames, decode_repeats
    h, e, l, o = (LETTERS[c] for c in 'helo')
    path = [h, h, e, l, l, l, 0, 0, o]                 # "hel_o" held for several frames
    labs, firsts = collapse_frames(path)
    assert labs == [h, e, l, 0, o] and firsts == [0, 2, 3, 6, 8]
    assert decode_repeats(labs) == _ids('hello')
    assert decode_repeats(collapse_frames([0, 0, h, 0, h, e])[0]) == _ids('hhhe')       # a leading repeat is dropped
    assert decode_repeats(collapse_frames([l, 0, l, 0])[0]) == _ids('llll')
    assert collapse_frames([]) == ([], []) and decode_repeats([]) == []
    assert decode_repeats([0]) == []


def test_transcript_with_the_repeat_index_raises():
    from wav2letter_pytorch_amd.asg import encode_repeats
    with pytest.raises(ValueError):
        encode_repeats([3, 0, 4])
    with pytest.raises(ValueError):
        encode_repeats([3, 5, 4], repeat=5)
    assert encode_repeats([3, 3, 0], repeat=5) == [3, 5, 0]


def _case(seed, T=4, A=3):
    g = np.random.default_rng(seed)
    return g.standard_normal((T, A)) * 2.0, g.standard_normal((A, A))


@pytest.mark.parametrize('y', [[1], [2, 0], [1, 2], [1, 0, 1, 2], [2, 1, 2, 0]])
def test_reference_recursions_equal_brute_force(y):
    """A = 3, T = 4: 81 paths.  Targets of length 1, 2 and 4 (= T: exactly one path), nonzero random transitions."""
    for seed in (0, 1):
        x, g = _case(seed)
        zf, zt, _, _ = R.brute_force(x, g, y)
        xt, gt = torch.from_numpy(x), torch.from_numpy(g)
        assert abs(float(R.full_logz(xt, gt)) - zf) < 1e-12
        assert abs(float(R.target_logz(xt, gt, y)) - zt) < 1e-12
        if len(y) == 4:
            assert abs(zt - R.path_score(x, g, y)) < 1e-12


def test_reference_gradients_are_posterior_differences():
    """the autograd gradients of the reference are the differences of posteriors the issue defines: every frame's row of
    d loss / d x sums to 0 (both posteriors sum to 1), and d loss / d g sums to 0 over all (i, j) per transition step"""
    x, g = _case(3, T=5, A=3)
    ref = R.asg_loss(x[None], g, [[1, 1, 2]], [5], reduction='sum')
    assert np.abs(ref['grad_x'][0].sum(axis=1)).max() < 1e-12
    assert abs(ref['grad_g'].sum()) < 1e-12
    assert ref['nll'][0] > 0 and abs(ref['loss'] - ref['nll'][0]) < 1e-12
    mean = R.asg_loss(x[None], g, [[1, 1, 2]], [5], reduction='mean')
    assert abs(mean['loss'] - ref['loss'] / 3) < 1e-12
    # infeasible: more labels than frames, and the empty transcript
    bad = R.asg_loss(np.stack([x, x]), g, [[1, 2, 1, 2, 1, 2], []], [5, 5])
    assert bad['loss'] == 0.0 and not bad['grad_x'].any() and not bad['grad_g'].any()


def test_reference_viterbi_equals_brute_force_best_path():
    for seed in (0, 1, 2):
        x, g = _case(seed)
        _, _, best, score = R.brute_force(x, g)
        path, s, margin = R.viterbi(x, g)
        assert path == best and abs(s - score) < 1e-12 and margin > 0
    # zero transitions: the per-frame argmax
    x, _ = _case(5)
    assert R.viterbi(x, np.zeros((3, 3)))[0] == np.argmax(x, axis=1).tolist()
    # a constructed tie: labels 0 and 2 score the same everywhere -> lowest final label, lowest predecessor
    x = np.array([[1.0, 0.0, 1.0]] * 4)
    path, s, margin = R.viterbi(x, np.zeros((3, 3)))
    assert path == [0, 0, 0, 0] and s == 4.0 and margin == 0.0
    assert R.brute_force(x, np.zeros((3, 3)))[2] == [0, 0, 0, 0]
    # a tie among predecessors only: the final label is unique, frame 0 ties between labels 1 and 2
    x = np.array([[0.0, 2.0, 2.0], [0.0, 0.0, 5.0]])
    assert R.viterbi(x, np.zeros((3, 3)))[0] == [1, 2] == R.brute_force(x, np.zeros((3, 3)))[2]


# ---- asg_ref: the float64 reference with per-element bounds that the direct GPU tests compare against -------------------------------

def _ref_rows(c, r):
    """the transcripts and lengths of a shared case as asg_loss takes them (clamped; a bad transcript contributes nothing)"""
    rows = [[int(v) for v in c.targets[n, :int(r['S'][n])]] if r['status'][n] != 2 else [] for n in range(c.dims[0])]
    return rows, [int(v) for v in r['Tn']]


SMALL = [k for k in R.CASES if k not in R.LONG]


@pytest.mark.parametrize('reduction', ['mean', 'sum'])
def test_asg_ref_agrees_with_the_autograd_reference(reduction):
    for name in SMALL:
        c = R.case(name)
        r = R.case_ref(name, reduction)
        rows, lens = _ref_rows(c, r)
        a = R.asg_loss(c.x, c.g, rows, lens, repeat=c.repeat, reduction=reduction)
        assert abs(a['loss'] - r['loss']) <= 1e-12 * max(1.0, abs(a['loss'])), name
        assert np.abs(a['nll'] - r['nll']).max() <= 1e-12 * max(1.0, np.abs(a['nll']).max()), name
        assert np.abs(a['grad_x'] - r['grad_x']).max() < 1e-11 and np.abs(a['grad_g'] - r['grad_g']).max() < 1e-10, name
        for n in range(c.dims[0]):
            assert not r['grad_x'][n, r['Tn'][n]:].any() and not r['grad_x_b'][n, r['Tn'][n]:].any()
            if r['status'][n]:
                assert r['nll'][n] == 0.0 and not r['grad_x'][n].any() and not r['grad_x_b'][n].any()


@pytest.mark.parametrize('raw,y', [([1], [1]), ([2, 2], [2, 0]), ([1, 2], [1, 2]), ([1, 1, 1, 2], [1, 0, 1, 2])])
def test_asg_ref_equals_brute_force(raw, y):
    for seed in (0, 1):
        x, g = _case(seed)
        zf, zt, _, _ = R.brute_force(x, g, y)
        r = R.asg_ref(x[None], g, np.array([raw], dtype=np.int32), [4], [len(raw)], 0, 'sum', len(raw))
        assert abs(r['nll'][0] - (zf - zt)) < 1e-12 and r['loss'] == r['nll'][0] and r['status'][0] == 0
        assert np.abs(r['grad_x'][0].sum(axis=1)).max() < 1e-12 and abs(r['grad_g'].sum()) < 1e-12


def test_asg_ref_closed_form_for_zero_scores():
    """x = 0, g = 0: every path weighs 1.  Z_full = T ln A; Z_tgt = ln C(T-1, S-1) (which S - 1 of the T - 1 steps advance); state s
    is occupied at frame t by C(t, s) C(T-1-t, S-1-s) of those paths: d loss / d x = 1 / A - the occupancy of the label's states"""
    from math import comb, log
    T, A, raw = 9, 4, [1, 2, 2, 3]
    y = R.encode(raw)
    S = len(y)
    assert y == [1, 2, 0, 3]
    r = R.asg_ref(np.zeros((1, T, A)), np.zeros((A, A)), np.array([raw], dtype=np.int32), [T], [S], 0, 'sum', S)
    assert abs(r['nll'][0] - (T * log(A) - log(comb(T - 1, S - 1)))) < 1e-12
    want = np.full((T, A), 1.0 / A)
    for t in range(T):
        for s in range(S):
            want[t, y[s]] -= comb(t, s) * comb(T - 1 - t, S - 1 - s) / comb(T - 1, S - 1)
    assert np.abs(r['grad_x'][0] - want).max() < 1e-13
    mean = R.asg_ref(np.zeros((2, T, A)), np.zeros((A, A)), np.array([raw, raw], dtype=np.int32), [T, T], [S, S], 0, 'mean', S)
    assert np.abs(mean['grad_x'][1] - want / (2 * S)).max() < 1e-14 and abs(mean['loss'] - r['nll'][0] / S) < 1e-13


def _worst(d, r):
    """the worst error / bound ratio of a defective result d over everything the GPU tests compare (inf: a status or an inf / NaN
    pattern differs)"""
    if d['status'].tolist() != r['status'].tolist():
        return np.inf
    worst = 0.0
    for k in ('nll', 'loss', 'grad_x', 'grad_g'):
        got, ref, b = np.asarray(d[k], dtype=np.float64), np.asarray(r[k], dtype=np.float64), np.asarray(r[k + '_b'])
        worst = max(worst, ratio(got, ref, b))
    return worst


@pytest.mark.parametrize('defect', [d for d in R.DEFECTS if d != 'grad_zero'])
def test_defect_leaves_the_bound(defect):
    names = [k for k in R.CASES if k[1:] in map(str, R.SPT_WIDTHS)] if defect == 'second_state_slot_lost' else SMALL
    hits = {}
    for name in names:
        for reduction in ('mean', 'sum'):
            w = _worst(R.case_ref(name, reduction, defect), R.case_ref(name, reduction))
            if w > 1.0:
                hits[f'{name}/{reduction}'] = w
    print(defect, 'leaves the bound on', len(hits), 'of', 2 * len(names), 'cases:',
          ', '.join(f'{k} {v:.3g}' for k, v in list(hits.items())[:6]))
    assert hits, f'{defect}: within the bound on every case of {names}'
    if defect == 'second_state_slot_lost':                   # the long cases are there for this fault: every one must see it
        assert len(hits) == 2 * len(names), hits


def test_zero_gradient_leaves_the_bound_on_every_feasible_case():
    """a kernel that wrote grad_x = 0: the flat 1e-3 bound let it pass wherever w_n = 1 / (N S) < 1e-3 (S = 1030, test_gpu_asg's
    two-states-per-thread case among them)"""
    for name in R.CASES:
        for reduction in ('mean', 'sum'):
            r = R.case_ref(name, reduction)
            if (r['status'] != 0).all():
                assert not r['grad_x'].any(), name
                continue
            w = ratio(np.zeros_like(r['grad_x']), r['grad_x'], r['grad_x_b'])
            print(f'grad_zero {name}/{reduction}: ratio {w:.3g}')
            assert w > 1.0, f'{name}/{reduction}: a zero gradient stays within the bound (ratio {w:.3g})'
    r = R.old_case_ref('spt2', 'mean')
    assert np.abs(r['grad_x']).max() < 1e-3                  # the old bound could not fail here ...
    w = ratio(np.zeros_like(r['grad_x']), r['grad_x'], r['grad_x_b'])
    assert w > 1.0, w                                        # ... the derived one can
    print(f'grad_zero spt2/mean: ratio {w:.3g}')


OLD = [(n, red, sc) for n in ('main', 'a29', 'a33', 'chunks', 'long') for red in ('mean', 'sum') for sc in ((1.0, 1.0), (30.0, 10.0))
       if sc == (1.0, 1.0) or n in ('main', 'a33')]
FLAT_GX_NOT_IMPLIED = {('a29', 'sum', (1.0, 1.0)), ('chunks', 'sum', (1.0, 1.0)), ('long', 'sum', (1.0, 1.0)),
                       ('main', 'sum', (30.0, 10.0)), ('a33', 'sum', (30.0, 10.0))}


def test_derived_bound_against_the_flat_bounds_of_the_old_cases():
    """on test_gpu_asg.py's cases the derived loss bound is below 1e-4 relative everywhere, and the derived grad_x bound below 1e-3
    everywhere under 'mean'.  Under 'sum' (w_n = 1) a worst-case bound of a posterior at T >= 40, or at emissions x 30, is above
    1e-3 on the cases listed: there the flat assertion is the sharper one, and _compare keeps both on every case."""
    not_implied = set()
    for name, reduction, scale in OLD:
        r = R.old_case_ref(name, reduction, scale)
        assert r['loss_b'] <= 1e-4 * abs(r['loss']), (name, reduction, scale)
        assert (r['nll_b'] <= 1e-4 * np.maximum(np.abs(r['nll']), 1.0)).all(), (name, reduction, scale)
        print(name, reduction, scale, f"grad_x bound {r['grad_x_b'].max():.3g}, loss bound / loss {r['loss_b'] / abs(r['loss']):.3g}")
        if r['grad_x_b'].max() > 1e-3:
            not_implied.add((name, reduction, scale))
    assert not_implied == FLAT_GX_NOT_IMPLIED


def test_case_table_reaches_every_kernel():
    variants = {name: R.case(name).variant for name in R.CASES}
    assert {v[:3] for v in variants.values()} == {(ap, nt, spt) for ap in (32, 64) for nt, spt in
                                                  ((64, 1), (128, 1), (256, 1), (512, 1), (1024, 1), (1024, 2), (1024, 4))}
    assert variants['S2049'][:3] == (32, 1024, 4) and variants['S2048'][:3] == (32, 1024, 2)        # spt 3 is rounded up to 4
    assert variants['A64-S4095'] == (64, 1024, 4, 114932) and variants['A64-S4095'][3] > 64 * 1024  # the big-LDS branch
    assert variants['A64-S513'][:3] == (64, 1024, 1)
    assert [min(R.TCH, R.TP_MAX // s) for s in (127, 128, 129, 4095)] == [64, 64, 63, 2]             # frames per posterior pass
    for name in R.CASES:
        c = R.case(name)
        N, T, A = c.dims
        assert c.x.dtype == np.float32 and c.g.shape == (A, A) and c.targets.shape == (N, max(c.Smax, 1))
        if name in R.LONG:
            assert T > 300 and c.x.max() <= 0.0 and np.abs(c.g).max() < 1.0
    # statuses 0, 1 and 2 in one launch; the clamps
    assert R.case_ref('S1024', 'mean')['status'].tolist() == [0, 0, 1, 1]
    assert R.case_ref('bad-repeat-r5', 'mean')['status'].tolist() == [0, 2, 0]
    r = R.case_ref('clamps', 'mean')
    assert r['S'].tolist() == [6, 4, 3] and r['Tn'].tolist() == [14, 14, 0] and r['status'].tolist() == [0, 0, 1]
    assert R.case('clamps').tg_len.tolist() == [9, 4, 3] and R.case('clamps').in_len.tolist() == [14, 99, -3]
    # a run of equal letters across every thread-count boundary of the long transcripts
    row = R.case('S4095').targets[0]
    for b in R.BOUNDARIES:
        assert len(set(row[b - 2:b + 2].tolist())) == 1
    enc = R.encode(row.tolist())
    assert enc[1022:1026] == [row[1022], 0, row[1022], 0]


def test_integer_viterbi_cases_rest_on_ties():
    """the inputs of the exact Viterbi test: every score an integer (exact in fp32), and with more than one label every reference
    path passes at least one decision with margin 0, so the device's tie rule decides the path"""
    for A in R.VITERBI_A:
        for T in R.VITERBI_T:
            x, g, in_len, refs, refs_full = R.viterbi_case(A, T)
            assert np.array_equal(x, np.round(x)) and np.array_equal(g, np.round(g)) and np.abs(x).max() <= 3 and np.abs(g).max() <= 3
            assert in_len.tolist() == [T, 0, 1, max(T - 3, 1)]
            for n, (path, score, margin), tn in [(n, refs[n], in_len[n]) for n in range(4)] + [(n, refs_full[n], T) for n in range(4)]:
                assert len(path) == tn and score == round(score) and abs(score) < 2 ** 24
                if tn:
                    assert score == R.path_score(x[n].astype(np.float64), g.astype(np.float64), path)
                    assert margin == 0.0 or A == 1, (A, T, n, tn)
    x, g, _, refs, _ = R.viterbi_case(5, 2)
    assert refs[2][0] == [0]                                 # labels 0 and 1 tie at frame 0: the lowest final label


def test_workspace_queries_answer_on_the_host():
    from wav2letter_pytorch_amd._lib import lib
    for N, T, A, Smax in [(1, 1, 1, 0), (2, 10, 29, 3), (3, 64, 5, 64), (3, 65, 33, 65), (1, 4101, 5, 4095), (2, 70, 64, 4095),
                          (7, 129, 64, 513), (1, 1 << 20, 2, 1)]:
        Sp = max(Smax, 1)
        want = 4 * (2 * N * T * A + 2 * N * T * Sp + N * Sp + 2 * N + N * -(-T // 64) * A * A)
        assert lib.w2l_asg_workspace_bytes(N, T, A, Smax) == want == R.asg_workspace_bytes(N, T, A, Smax)
        assert lib.w2l_asg_viterbi_workspace_bytes(N, T, A) == N * T * (32 if A <= 32 else 64)
    for bad in [(0, 10, 5, 3), (2, 0, 5, 3), (2, (1 << 20) + 1, 5, 3), (2, 10, 0, 3), (2, 10, 65, 3), (2, 10, 5, -1), (2, 10, 5, 4096)]:
        assert lib.w2l_asg_workspace_bytes(*bad) == -1, bad
    for bad in [(0, 10, 5), (2, 0, 5), (2, (1 << 20) + 1, 5), (2, 10, 0), (2, 10, 65)]:
        assert lib.w2l_asg_viterbi_workspace_bytes(*bad) == -1, bad


def test_config_key_model_criterion(tmp_path):
    from wav2letter_pytorch_amd.config import criterion_name, load_config, to_cfg
    from wav2letter_pytorch_amd.defaults import wav2letter_model
    from wav2letter_pytorch_amd.train import build_config
    assert criterion_name(wav2letter_model(1)) == 'ctc'
    assert criterion_name(to_cfg({'name': 'wav2letter'})) == 'ctc'           # an older config without the key
    assert 'criterion' not in build_config([]).model and criterion_name(build_config([]).model) == 'ctc'
    assert criterion_name(build_config(['model.criterion=asg']).model) == 'asg'
    with pytest.raises(ValueError, match='ctc and asg'):
        build_config(['model.criterion=mmi'])
    # the YAML tree of the reference with the override syntax
    (tmp_path / 'model').mkdir()
    (tmp_path / 'config.yaml').write_text('defaults:\n  - model: wav2letter\ntrainer:\n  gpus: 0\n')
    (tmp_path / 'model' / 'wav2letter.yaml').write_text('# @package model\nname: wav2letter\nmid_layers: 1\n')
    assert 'criterion' not in load_config(str(tmp_path)).model          # unset stays unset: the config a default run saves is unchanged
    assert criterion_name(load_config(str(tmp_path)).model) == 'ctc'
    assert load_config(str(tmp_path), ['model.criterion=asg']).model.criterion == 'asg'
    with pytest.raises(ValueError, match='ctc and asg'):
        load_config(str(tmp_path), ['model.criterion=viterbi'])
    (tmp_path / 'model' / 'wav2letter.yaml').write_text('# @package model\nname: wav2letter\ncriterion: asg\n')
    assert load_config(str(tmp_path)).model.criterion == 'asg'


def test_default_model_keeps_ctc_and_its_state_dict():
    from wav2letter_pytorch_amd import Wav2Letter
    from wav2letter_pytorch_amd.asg import ASGDecoder, ASGLoss
    from wav2letter_pytorch_amd.ctc_loss import CTCLoss
    from wav2letter_pytorch_amd.decoder import GreedyDecoder
    from wav2letter_pytorch_amd.defaults import wav2letter_model
    cfg = wav2letter_model(2)
    torch.manual_seed(3)
    m = Wav2Letter(cfg)
    assert type(m.criterion) is CTCLoss and type(m.ctc_decoder) is GreedyDecoder
    keys = list(m.state_dict())
    assert not any('criterion' in k for k in keys)
    assert 'criterion' not in cfg                      # the default config does not carry the key
    cfg['criterion'] = 'ctc'                           # ... and naming the default builds the same model
    torch.manual_seed(3)
    old = Wav2Letter(cfg)
    assert list(old.state_dict()) == keys and type(old.criterion) is CTCLoss
    assert torch.equal(old.example_input_array[0], m.example_input_array[0])
    cfg['criterion'] = 'asg'
    a = Wav2Letter(cfg)
    assert isinstance(a.criterion, ASGLoss) and isinstance(a.ctc_decoder, ASGDecoder)
    assert sorted(a.state_dict()) == sorted(keys + ['criterion.transitions'])
    g = a.criterion.transitions
    assert tuple(g.shape) == (29, 29) and g.dtype == torch.float32 and not g.detach().any()
    assert any(p is g for p in a.parameters())        # configure_optimizers hands it to the optimizer
    cfg['criterion'] = 'mmi'
    with pytest.raises(ValueError, match='ctc and asg'):
        Wav2Letter(cfg)


def test_jasper_refuses_asg():
    """Jasper's infer() returns probabilities, its training forward log-probabilities: transitions learned on one scale must
    not silently decode the other"""
    from wav2letter_pytorch_amd import Jasper
    from wav2letter_pytorch_amd.defaults import jasper_model
    cfg = jasper_model(1)
    assert 'criterion' not in cfg
    cfg['criterion'] = 'asg'
    with pytest.raises(NotImplementedError, match='Wav2Letter'):
        Jasper(cfg)


def test_asg_refuses_cpu_tensors_and_too_many_labels():
    from wav2letter_pytorch_amd._lib import W2LError, lib
    from wav2letter_pytorch_amd.asg import ASGDecoder, ASGLoss
    crit = ASGLoss(5)
    with pytest.raises(W2LError):
        crit(torch.zeros(4, 1, 5), torch.ones(1, 2, dtype=torch.int32), torch.tensor([4]), torch.tensor([2]))
    with pytest.raises(ValueError):
        ASGLoss(65)
    with pytest.raises(ValueError):
        ASGDecoder([str(i) for i in range(65)])
    with pytest.raises(NotImplementedError):
        ASGLoss(5, reduction='none')
    # the workspace queries answer on the host: -1 out of range
    assert lib.w2l_asg_workspace_bytes(2, 10, 65, 3) == -1 and lib.w2l_asg_workspace_bytes(2, 10, 29, 4096) == -1
    assert lib.w2l_asg_viterbi_workspace_bytes(2, 10, 65) == -1
    assert lib.w2l_asg_workspace_bytes(2, 10, 29, 3) > 0 and lib.w2l_asg_viterbi_workspace_bytes(2, 10, 29) == 2 * 10 * 32
    assert lib.w2l_replay_op(b'w2l_asg_loss') >= 0


def test_out_of_scope_requests_fail_loudly_in_the_test_cli():
    from wav2letter_pytorch_amd.test import build_config
    base = ['model_path=x.ckpt', 'data.test_manifest=t.csv', 'model.criterion=asg']
    assert build_config(base).decoder == 'greedy'
    with pytest.raises(NotImplementedError, match='beam'):
        build_config(base + ['decoder=beam'])
    with pytest.raises(NotImplementedError, match='word_times'):
        build_config(base + ['word_times=true'])
    with pytest.raises(NotImplementedError, match='data parallelism'):
        from wav2letter_pytorch_amd.train import main
        main(['data.train_manifest=a.csv', 'data.val_manifest=b.csv', 'model.criterion=asg', 'trainer.gpus=2'])
