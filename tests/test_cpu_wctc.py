"""Wildcard CTC, host side (no GPU): the float64 reference the GPU tests compare against (tests/wctc_refs.py) pinned by a
brute-force sum over every state path, by torch's own CTC where no star stands, and by torch autograd through a float64
restatement of the recursion; the embedding inequality W-CTC exists for; the bound shown to have teeth against every planted
defect on cases the GPU tests run; the parsing rule; and the plumbing from the manifest's mark to the criterion and the metrics."""
import itertools
import json
import wave

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import frontend_refs as FR
import wctc_refs as R
from direct_helpers import ratio

STAR, BLANK = 4, 0            # the small problems here: C = 4 classes, star = C


def raw_row(z, w):
    """labels z and gap flags w (len(z) + 1) -> a raw row"""
    row = [STAR] * int(w[0])
    for i, v in enumerate(z):
        row += [v] + [STAR] * int(w[i + 1])
    return row


def ref_one(lp, row, penalty, Tn=None, star=STAR, width=None, **kw):
    T = lp.shape[0]
    width = max(len(row), 1) if width is None else width
    tg = np.full((1, width), -7, dtype=np.int32)
    tg[0, :len(row)] = row
    return R.wctc_ref(lp[None], tg, [T if Tn is None else Tn], [len(row)], BLANK, 0, width, star, penalty, **kw)


def rand_lp(rng, T, C=4):
    x = rng.standard_normal((T, C))
    return x - np.log(np.exp(x).sum(axis=1, keepdims=True))


# ---- brute force: every state path of the definition ---------------------------------------------------------------------------------

def brute(lp, z, w, penalty):
    """(nll, grad wrt logits) by enumerating every path over the L = 2S + 1 states: starts in 0 or 1, ends in L-1 or L-2, moves
    s -> s, s -> s+1, and s -> s+2 onto a label state whose label differs from the one two states back"""
    T, C = lp.shape
    S = len(z)
    L = 2 * S + 1
    total = 0.0
    post, omega = np.zeros((T, C)), np.zeros(T)
    for path in itertools.product(range(L), repeat=T):
        if path[0] > 1 or path[-1] < L - 2:
            continue
        ok = True
        for a, b in zip(path, path[1:]):
            d = b - a
            if d not in (0, 1, 2) or (d == 2 and not ((b & 1) and z[b >> 1] != z[(b >> 1) - 1])):
                ok = False
                break
        if not ok:
            continue
        p = 1.0
        for t, s in enumerate(path):
            p *= np.exp(lp[t, z[s >> 1]]) if s & 1 else (np.exp(penalty) if w[s >> 1] else np.exp(lp[t, BLANK]))
        total += p
        for t, s in enumerate(path):
            if s & 1:
                post[t, z[s >> 1]] += p
            elif w[s >> 1]:
                omega[t] += p
            else:
                post[t, BLANK] += p
    if total == 0.0:
        return np.inf, None
    post, omega = post / total, omega / total
    return -np.log(total), (np.exp(lp) * (1 - omega[:, None]) - post) / max(S, 1)


@pytest.mark.parametrize('z', [[], [1], [1, 2], [2, 2]], ids=str)
def test_reference_equals_the_sum_over_all_paths(z):
    rng = np.random.default_rng(11 + len(z) + sum(z))
    checked = 0
    for T in range(1, 6):
        lp = rand_lp(rng, T)
        for w in itertools.product((0, 1), repeat=len(z) + 1):
            for penalty in (0.0, -0.5):
                want_nll, want_grad = brute(lp, z, w, penalty)
                r = ref_one(lp, raw_row(z, w), penalty)
                if not np.isfinite(want_nll):
                    assert np.isinf(r['nll'][0]) and r['status'][0] == 1
                    continue
                assert r['status'][0] == 0 and abs(r['nll'][0] - want_nll) < 1e-12, (T, w, penalty)
                assert np.abs(r['grad'][0] - want_grad).max() < 1e-12, (T, w, penalty)
                assert np.abs(r['grad'][0].sum(axis=1)).max() < 1e-12          # sums to zero over the classes
                checked += 1
    assert checked >= 5


def test_score_is_not_a_probability():
    """one frame, the row '*': the single state emits exp(penalty) whatever the frame holds -- nll = -penalty, 0 at penalty 0,
    and a star beside a label makes nll negative where the label's own probability is counted twice"""
    lp = np.log(np.array([[0.05, 0.9, 0.03, 0.02]]))
    assert ref_one(lp, [STAR], 0.0)['nll'][0] == 0.0
    assert ref_one(lp, [STAR], -0.5)['nll'][0] == 0.5
    two = np.log(np.array([[0.05, 0.9, 0.03, 0.02]] * 2))
    assert ref_one(two, [STAR, 1, STAR], 0.0)['nll'][0] < 0.0                  # (*,1), (1,*), (1,1): 0.9 + 0.9 + 0.81 > 1


# ---- no star: torch's CTC ---------------------------------------------------------------------------------------------------------

def test_without_stars_it_is_torch_ctc():
    rng = np.random.default_rng(21)
    N, T, C, Smax = 4, 30, 7, 9
    logits = torch.tensor(rng.standard_normal((N, T, C)), dtype=torch.float64, requires_grad=True)
    lens = [9, 5, 1, 0]
    tg = np.zeros((N, Smax), dtype=np.int32)
    for n, s in enumerate(lens):
        tg[n, :s] = rng.integers(1, C, size=s)
    tg[0, :4] = [3, 3, 3, 2]
    in_len = [30, 22, 17, 30]
    lp = F.log_softmax(logits, dim=2)
    want = F.ctc_loss(lp.transpose(0, 1), torch.tensor(tg, dtype=torch.long), torch.tensor(in_len), torch.tensor(lens), blank=0,
                      reduction='mean', zero_infinity=False)
    want.backward()
    for penalty in (0.0, -0.5):                           # no wildcard gap: the penalty touches nothing
        r = R.wctc_ref(lp.detach().numpy(), tg, in_len, lens, 0, 0, Smax, C, penalty)
        assert abs(r["loss"] - float(want.detach())) < 1e-12 and not r["status"].any()
        assert np.abs(r['grad'] - logits.grad.numpy()).max() < 1e-12
    c = FR.ctc_ref(lp.detach().numpy(), tg, in_len, lens, 0, 0, Smax)
    assert np.array_equal(c['nll'], r['nll']) and np.array_equal(c['grad'], r['grad'])     # and the CTC reference, value for value


# ---- torch autograd through a restatement of the recursion ------------------------------------------------------------------------------

NEG = -1e30      # stands for log 0: finite, so that autograd never meets inf - inf


def torch_wctc(logits, rows, in_len, blank, star, penalty):
    """mean_n(nll_n / max(S_n, 1)) of float64 logits [N][T][C], by the alpha recursion with torch.logsumexp"""
    lp = F.log_softmax(logits, dim=2)
    terms = []
    for n, row in enumerate(rows):
        z, w, bad = R.parse_row(row, len(row), star, logits.shape[2], blank)
        assert not bad
        S, L, Tn = len(z), 2 * len(z) + 1, in_len[n]
        ext = [int(z[s >> 1]) if s & 1 else blank for s in range(L)]
        wild = torch.tensor([(not s & 1) and bool(w[s >> 1]) for s in range(L)])
        skip = torch.tensor([bool(s & 1) and s >= 3 and ext[s] != ext[s - 2] for s in range(L)])
        pen = torch.full((L,), float(penalty), dtype=torch.float64)
        neg = torch.full((L,), NEG, dtype=torch.float64)
        em = torch.where(wild[None, :], pen[None, :], lp[n][:, ext])
        alpha = torch.where(torch.arange(L) <= 1, em[0], neg)
        for t in range(1, Tn):
            a1 = torch.cat([neg[:1], alpha[:-1]])
            a2 = torch.where(skip, torch.cat([neg[:2], alpha[:-2]])[:L], neg)
            alpha = torch.logsumexp(torch.stack([alpha, a1, a2]), dim=0) + em[t]
        terms.append(-torch.logsumexp(alpha[max(L - 2, 0):], dim=0) / max(S, 1))
    return torch.stack(terms).mean()


def test_gradient_equals_autograd_through_the_recursion():
    rng = np.random.default_rng(31)
    C, T = 6, 14
    star = C
    rows = [[star, 1, 2, star, 2, 3], [4, star, star, 4, 4, star], [star], [2, 5, 1], [star, 3, star, 3, star, 3, star]]
    in_len = [14, 11, 9, 14, 12]
    N = len(rows)
    width = max(len(r) for r in rows)
    tg = np.full((N, width), -7, dtype=np.int32)
    for n, r in enumerate(rows):
        tg[n, :len(r)] = r
    for penalty in (0.0, -0.5):
        logits = torch.tensor(rng.standard_normal((N, T, C)) * 2, dtype=torch.float64, requires_grad=True)
        loss = torch_wctc(logits, rows, in_len, 0, star, penalty)
        loss.backward()
        lp = F.log_softmax(logits.detach(), dim=2).numpy()
        r = R.wctc_ref(lp, tg, in_len, [len(x) for x in rows], 0, 0, width, star, penalty)
        assert abs(r["loss"] - float(loss.detach())) < 1e-12
        assert np.abs(r['grad'] - logits.grad.numpy()).max() < 1e-12
        for n in range(N):
            assert not r['grad'][n, in_len[n]:].any()


# ---- what the wildcard is for -----------------------------------------------------------------------------------------------------

def test_embedding_inequality():
    """junk frames around an utterance: every CTC path of z over the inner frames, with the junk frames in the wildcards, is a
    path of '* z *' over all frames of at least its weight (a wildcard frame has weight 1 >= any probability), and the map is
    one to one: nll(* z *, whole) <= nll_ctc(z, inner) at penalty 0 -- no tolerance, in float64"""
    rng = np.random.default_rng(41)
    C = 7
    for trial in range(20):
        S = int(rng.integers(0, 5))
        z = [int(v) for v in rng.integers(1, C, size=S)]
        reps = sum(a == b for a, b in zip(z, z[1:]))
        Tin = S + reps + int(rng.integers(1, 6))
        pre, post = int(rng.integers(0, 6)), int(rng.integers(0, 6))
        whole = rand_lp(rng, pre + Tin + post, C) * 2
        whole = whole - np.log(np.exp(whole).sum(axis=1, keepdims=True))
        inner = whole[pre: pre + Tin]
        ctc = ref_one(inner, z, 0.0, star=C, want_grad=False)['nll'][0]
        wild = ref_one(whole, [C] + z + [C], 0.0, star=C, want_grad=False)['nll'][0]
        assert np.isfinite(ctc) and wild <= ctc, (trial, wild, ctc)
        # and the plain CTC of z over the whole recording has to explain the junk with z's labels and blanks
        assert wild <= ref_one(whole, z, 0.0, star=C, want_grad=False)['nll'][0]


# ---- parsing ----------------------------------------------------------------------------------------------------------------------

def test_parsing_rule():
    s = 9
    z, w, bad = R.parse_row([s, s, 1, 2, s, s, s, 2, s], 9, s, 9, 0)
    assert z.tolist() == [1, 2, 2] and w.tolist() == [True, False, True, True] and not bad        # consecutive stars are one
    z, w, bad = R.parse_row([s, s, s], 3, s, 9, 0)
    assert z.tolist() == [] and w.tolist() == [True] and not bad                                  # star-only: S = 0, w_0 = 1
    z, w, bad = R.parse_row([], 0, s, 9, 0)
    assert z.tolist() == [] and w.tolist() == [False] and not bad                                 # empty: the all-blank path
    z, w, bad = R.parse_row([1, 2, s, 5], 2, s, 9, 0)
    assert z.tolist() == [1, 2] and w.tolist() == [False, False, False]                           # padding beyond R is ignored
    for row in ([1, 0, 2], [1, 10], [-1]):
        assert R.parse_row(row, len(row), s, 9, 0)[2]                                             # blank, past the star, negative
    rng = np.random.default_rng(51)
    lp = rand_lp(rng, 6, 9)
    for penalty in (0.0, -0.5):
        r = ref_one(lp, [s, s, s], penalty, star=s)
        assert abs(r['nll'][0] + 6 * penalty) < 1e-15 and not r['grad'].any()    # omega == 1: nothing reaches the logits
        assert ref_one(lp, [s], penalty, star=s)['nll'][0] == r['nll'][0]
        e = ref_one(lp, [], penalty, star=s)
        assert abs(e['nll'][0] + lp[:, 0].sum()) < 1e-12 and e['S'][0] == 0
        a, b = ref_one(lp, [s, s, 1, 2, s, s, s, 2, s], penalty, star=s), ref_one(lp, [s, 1, 2, s, 2, s], penalty, star=s)
        assert a['nll'][0] == b['nll'][0] and np.array_equal(a['grad'], b['grad']) and a['S'][0] == b['S'][0] == 3
    assert R.wctc_ref(lp[None], np.array([[1, 0, 2]], dtype=np.int32), [6], [3], 0, 0, 3, s, 0.0)['status'][0] == 2


# ---- the bound has teeth ------------------------------------------------------------------------------------------------------------

def caught(got, ref, bound):
    ok, g, r = FR.split_nonfinite(got, ref)
    return (not ok) or ratio(g, r, np.where(np.isfinite(bound), bound, 0.0)) > 1.0


def small_shared_cases():
    cases = [R.shape_case(s, g, p) for s, g, p in R.shape_cases() if R.SHAPES[s][0] in ('L63', 'L65')]
    return cases + [R.infeasible_case(1)]


@pytest.mark.parametrize('defect', R.DEFECTS)
def test_defect_exceeds_bound(defect):
    hits = []
    for c in small_shared_cases():
        r, d = R.case_ref(c), R.case_ref(c, defect)
        m = ~np.isnan(r['grad'])
        if caught(d['nll'], r['nll'], r['nll_b']) or caught(d['grad'][m], r['grad'][m], r['grad_b'][m]):
            hits.append(c.name)
    assert hits, defect
    print(defect, len(hits), hits[:4])


def test_shared_cases_are_what_the_issue_names():
    """every dispatch edge is reached, every row feasible, no zero bound under a non-zero reference; the bounds of the short rows
    are tight"""
    variants = {R.SHAPES[s][0]: R.shape_case(s, 0, 0.0).variant for s in range(len(R.SHAPES))}
    assert variants == {'L63': (64, 1, True), 'L65': (128, 1, True), 'L129': (192, 1, True), 'L1025': (1024, 2, True),
                        'mem': (64, 1, False)}
    for s, g, p in R.shape_cases():
        if R.SHAPES[s][0] in ('L1025', 'mem') and (g, p) != (1, -0.5):
            continue                                          # (the long references are computed once, by the GPU tests)
        c = R.shape_case(s, g, p)
        r = R.case_ref(c)
        assert not r['status'].any() and np.isfinite(r['nll']).all(), c.name
        assert (r['grad_b'][r['grad'] != 0] > 0).all()
        assert len(set(c.in_len.tolist())) == 3 and c.in_len.max() == c.dims[1]
    r = R.case_ref(R.shape_case(0, 1, -0.5))
    assert (r['nll_b'] < 2e-3).all()                          # 56 steps of u (K1 |alpha| + K2), |alpha| <= 56 * ~4.5
    b = R.case_ref(R.bad_entry_case())
    assert b['status'].tolist() == [0, 2, 2, 2, 0] and not b['grad'][1:4].any() and not b['nll'][1:4].any()
    for zi in (0, 1):
        f = R.case_ref(R.infeasible_case(zi))
        assert f['status'].tolist() == [1, 1, 0, 1]
        assert np.isinf(f['nll'][[0, 1, 3]]).all() != bool(zi) and np.isfinite(f['nll'][2])


# ---- host plumbing -------------------------------------------------------------------------------------------------------------------

class _NoExtractor:
    def __init__(self, *a, **k):
        pass


def _manifest(tmp_path, texts):
    rows = []
    for i, text in enumerate(texts):
        path = tmp_path / f'u{i}.wav'
        with wave.open(str(path), 'wb') as w:
            w.setnchannels(1)
            w.setsampwidth(2)
            w.setframerate(16000)
            w.writeframes(np.zeros(4000, dtype='<i2').tobytes())
        rows.append(dict(audio_filepath=str(path), text=text))
    man = str(tmp_path / 'm.json')
    with open(man, 'w') as f:
        f.write('\n'.join(json.dumps(r) for r in rows) + '\n')
    return man


CONF = dict(window='hamming', window_stride=0.01, window_size=0.02, sample_rate=16000)


def test_dataset_targets(tmp_path, monkeypatch):
    from wav2letter_pytorch_amd.data import data_loader as DL
    monkeypatch.setattr(DL, 'SpectrogramExtractor', _NoExtractor)            # (the extractor needs a GPU; nothing here extracts)
    labels = list('_ab ')
    man = _manifest(tmp_path, ['ab * ba', '*a', 'a?b_'])
    plain = DL.SpectrogramDataset(man, CONF, labels)
    assert plain._target('ab * ba') == [1, 2, 3, 3, 2, 1] and plain.wildcard is None       # as today: an unknown character is dropped
    ds = DL.SpectrogramDataset(man, CONF, labels, wildcard='*')
    assert ds._target('ab * ba') == [1, 2, 3, 4, 3, 2, 1]                    # the mark is len(labels)
    assert ds._target('*a') == [4, 1] and ds._target('a?b_') == [1, 2] and ds._target('') == []
    assert ds.raw(1)[1] == [4, 1] and ds.raw(1)[3] == '*a'
    ends = DL.SpectrogramDataset(man, CONF, labels, wildcard='*', wildcard_ends=True)
    assert ends._target('ab') == [4, 1, 2, 4] and ends._target('') == [4, 4] and ends._target('*a') == [4, 4, 1, 4]
    for kw in (dict(wildcard='a'), dict(wildcard='**'), dict(wildcard_ends=True)):
        with pytest.raises(ValueError):
            DL.SpectrogramDataset(man, CONF, labels, **kw)


def test_loaders_thread_the_keys(tmp_path, monkeypatch):
    from wav2letter_pytorch_amd import train as T
    from wav2letter_pytorch_amd.config import wildcard_options
    from wav2letter_pytorch_amd.data import data_loader as DL
    monkeypatch.setattr(DL, 'SpectrogramExtractor', _NoExtractor)
    man = _manifest(tmp_path, ['ab', 'b*a'])
    base = [f'data.train_manifest={man}', f'data.val_manifest={man}']
    labels = list('_ab ')
    cfg = T.build_config(base)
    assert 'wildcard' not in cfg.model and wildcard_options(cfg.model) == (None, 0.0)
    for loader in T.get_data_loaders(labels, cfg.data):
        assert loader._spect_ds.wildcard is None and not loader._spect_ds.wildcard_ends
    for mark in ('*', "'*'", '#'):                        # unquoted, as a shell hands it over, and quoted for YAML
        cfg = T.build_config(base + [f'model.wildcard={mark}', 'data.wildcard_ends=true', 'model.wildcard_penalty=-0.25'])
        assert wildcard_options(cfg.model, labels) == (mark.strip("'"), -0.25)
    for loader in T.get_data_loaders(labels, cfg.data, wildcard='#'):        # training and validation alike
        assert loader._spect_ds.wildcard == '#' and loader._spect_ds._target('a#') == [4, 1, 4, 4]
    with pytest.raises(ValueError, match='wildcard_ends'):
        T.get_data_loaders(labels, cfg.data)                                 # data.wildcard_ends needs model.wildcard


def test_config_errors():
    from wav2letter_pytorch_amd import train as T
    from wav2letter_pytorch_amd.config import wildcard_options
    from wav2letter_pytorch_amd.defaults import wav2letter_model
    with pytest.raises(NotImplementedError, match='asg'):
        T.build_config(['model.wildcard=*', 'model.criterion=asg'])
    with pytest.raises(ValueError, match='one character'):
        T.build_config(['model.wildcard=**'])
    cfg = wav2letter_model(1)
    cfg['labels'] = list("_'abcdefghijklmnopqrstuvwxyz ")
    cfg['wildcard'] = 'q'
    with pytest.raises(ValueError, match='labels'):
        wildcard_options(cfg)
    cfg['wildcard'] = '*'
    cfg['wildcard_penalty'] = 0.5
    with pytest.raises(ValueError, match='penalty'):
        wildcard_options(cfg)


def _labelled(cfg):
    from wav2letter_pytorch_amd.data import label_sets
    if type(cfg['labels']) is str:
        cfg['labels'] = list(label_sets.labels_map[cfg['labels']])
        cfg['decoder']['labels'] = cfg['labels']
    return cfg


def test_model_criterion_choice():
    from wav2letter_pytorch_amd import Wav2Letter
    from wav2letter_pytorch_amd.ctc_loss import CTCLoss, WildcardCTCLoss
    from wav2letter_pytorch_amd.decoder import GreedyDecoder
    from wav2letter_pytorch_amd.defaults import wav2letter_model
    cfg = _labelled(wav2letter_model(1))
    m = Wav2Letter(cfg)
    assert 'wildcard' not in cfg and m.wildcard is None
    assert type(m.criterion) is CTCLoss                   # a config without the key: the criterion of before, same arguments
    assert (m.criterion.blank, m.criterion.reduction, m.criterion.zero_infinity) == (0, 'mean', True)
    keys = list(m.state_dict())
    cfg['wildcard'] = '*'
    cfg['wildcard_penalty'] = -0.5
    w = Wav2Letter(cfg)
    assert type(w.criterion) is WildcardCTCLoss and w.wildcard == '*' and type(w.ctc_decoder) is GreedyDecoder
    assert (w.criterion.blank, w.criterion.reduction, w.criterion.zero_infinity, w.criterion.penalty) == (0, 'mean', True, -0.5)
    assert w.criterion.last_status() is None
    assert list(w.state_dict()) == keys                   # the output classes are unchanged: the wildcard lives in targets only
    assert w.ctc_decoder.labels == m.ctc_decoder.labels
    cfg['criterion'] = 'asg'
    with pytest.raises(NotImplementedError, match='asg'):
        Wav2Letter(cfg)
    del cfg['criterion']
    cfg['wildcard'] = 'e'
    with pytest.raises(ValueError, match='labels'):
        Wav2Letter(cfg)
    cfg['wildcard'] = '<*>'
    with pytest.raises(ValueError, match='one character'):
        Wav2Letter(cfg)
    with pytest.raises(ValueError, match='penalty'):
        WildcardCTCLoss(penalty=0.1)
    with pytest.raises(NotImplementedError):
        WildcardCTCLoss(reduction='sum')


def test_metric_text():
    from wav2letter_pytorch_amd import Wav2Letter
    from wav2letter_pytorch_amd.config import strip_wildcard
    from wav2letter_pytorch_amd.defaults import wav2letter_model
    assert strip_wildcard('* the cat * sat *', '*') == 'the cat sat'
    assert strip_wildcard('the*cat', '*') == 'the cat' and strip_wildcard('**', '*') == ''
    assert strip_wildcard('the  cat', '*') == 'the  cat' and strip_wildcard('a * b', None) == 'a * b'   # no mark: untouched
    cfg = _labelled(wav2letter_model(1))
    assert Wav2Letter(cfg).metric_texts(('a * b',)) == ('a * b',)
    cfg['wildcard'] = '*'
    m = Wav2Letter(cfg)
    assert m.metric_texts(('a * b', 'ab', '*')) == ['a b', 'ab', '']
    # the scorer sees the stripped reference: a perfect hypothesis of the transcribed part scores 0 errors
    assert m.ctc_decoder.wer_ratio(m.metric_texts(['* the cat *'])[0], 'the cat')[0] == 0
