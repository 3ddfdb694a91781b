"""w2l_ctc_align_long (csrc/ctc_align_long.hip) against the host model it restates (alignment.viterbi_align_host in float32: a
max is exact and the adds run along a path, so the score's bytes, the path, starts, ends and the -1 fills are the model's
however the trellis is cut), under forced plans that cross many seams at small shapes, the planner's candidates, the default
plan beyond each limit of w2l_ctc_align, and ``Decoder.align_long`` / ``model.align_transcript`` on top of it."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import align_long_refs as R  # noqa: E402

from wav2letter_pytorch_amd import alignment as AL  # noqa: E402
from wav2letter_pytorch_amd.alignment import ctc_forced_align, ctc_forced_align_long, viterbi_align_host  # noqa: E402

pytestmark = pytest.mark.gpu


def _row(res):
    """an Alignment with N = 1 as a HostAlignment"""
    assert res.paths.shape[0] == 1 and res.scores.shape == (1,)
    return AL.HostAlignment(res.scores[0], res.paths[0], res.starts[0], res.ends[0], bool(res.feasible[0]))


def _check(lp, tg, plan, blank=0):
    ref = viterbi_align_host(lp, tg, blank=blank, dtype=np.float32)
    got = _row(ctc_forced_align_long(lp, tg, blank=blank, plan=plan))
    assert got.path.shape == (lp.shape[0],) and got.starts.shape == got.ends.shape == (len(tg),)
    assert R.same(got, ref), (plan, got.score, ref.score)
    if not ref.feasible:
        assert got.score == -np.inf and (got.path == -1).all() and (got.starts == -1).all() and (got.ends == -1).all()
    return ref


# ------------------------------------------------------------------------------------------------------------ forced plans
@pytest.mark.parametrize('plan', R.SMALL_PLANS)
def test_forced_plan_over_the_grid_of_small_shapes(plan):
    """T in {1, 2, 16, 17, 70} x S in {0, 1, 31, 32, 33, 100}; (16, 64) at T = 70, S = 100 is five time blocks by four tiles"""
    feasible = [name for name, lp, tg in R.grid_cases() if _check(lp, tg, plan).feasible]
    assert len(feasible) >= 10 and 'grid T=70 S=33' in feasible and 'grid T=1 S=0' in feasible and 'grid T=70 S=100' not in feasible


@pytest.mark.parametrize('plan', R.SINGLE_PLANS)
def test_single_path(plan):
    """T = S + repeats, T = S, the staircase at an odd offset from the tiles (the input that needs the whole halo; (32, 64)
    and (32, 128) have a halo of exactly 2 tb states); one frame fewer: status 1 and -1 everywhere"""
    want = {'single T=S+repeats': True, 'single T=S+repeats-1': False, 'single T=S': True, 'single T=S-1': False,
            'single staircase+31': True}
    for name, lp, tg in R.single_path_cases():
        ref = _check(lp, tg, plan)
        assert ref.feasible == want[name], name
        if ref.feasible and 'repeats' not in name:
            assert ref.starts.tolist() == ref.ends.tolist() or name == 'single staircase+31'


def test_probability_input_with_zeros():
    """log_probs=False with exact zeros: one logf per emission read, so bit-equal to w2l_ctc_align on the same probabilities
    (same device logf), and the path spells the target"""
    rng = np.random.default_rng(7)
    t, a = 300, 29
    p = np.exp(R.log_probs(rng, t, a)).astype(np.float32)
    p[rng.random(p.shape) < 0.2] = 0.0
    p[:, 0] = np.maximum(p[:, 0], 1e-3)
    tg = R.target(rng, a, 60)
    for j, c in enumerate(tg):
        p[j::4, c] = np.maximum(p[j::4, c], 1e-2)
    old = ctc_forced_align(p, [tg], log_probs=False)
    assert old.feasible[0]
    for plan in ((16, 64), (32, 64), None):
        got = _row(ctc_forced_align_long(p, tg, log_probs=False, plan=plan))
        assert R.same(got, AL.HostAlignment(old.scores[0], old.paths[0], old.starts[0], old.ends[0], True)), plan
        prev = np.concatenate(([-1], got.path[:-1]))
        assert got.path[(got.path != prev) & (got.path != 0)].tolist() == tg
    p2 = p.copy()
    p2[7, :] = 0.0                                         # a frame no label can pass: no path, not an error
    got = _row(ctc_forced_align_long(p2, tg, log_probs=False, plan=(16, 64)))
    assert not got.feasible and got.score == -np.inf and (got.path == -1).all() and (got.starts == -1).all()


def test_bad_input_raises():
    rng = np.random.default_rng(9)
    lp = R.log_probs(rng, 70, 29)
    tg = R.target(rng, 29, 20)
    p = np.exp(lp)
    p[69, 28] = -1e-3
    for plan in ((16, 64), None):
        with pytest.raises(ValueError, match='negative probability'):
            ctc_forced_align_long(p, tg, log_probs=False, plan=plan)
    p[69, 28] = np.nan
    with pytest.raises(ValueError):
        ctc_forced_align_long(p, tg, log_probs=False)
    for v in (0, 29, -5, 1 << 20):
        bad = list(tg)
        bad[13] = v
        with pytest.raises(ValueError, match='outside'):
            ctc_forced_align_long(lp, bad, plan=(16, 64))
    _check(lp, tg, (16, 64))                               # the device is fine afterwards


def test_every_plan_the_planner_picks_from():
    """T = 300, S = 140, a non-zero blank: every candidate pair forced, and the default, bit-equal to ctc_forced_align"""
    rng = np.random.default_rng(5)
    lp = R.log_probs(rng, 300, 29, holes=0.03)
    tg = R.target(rng, 29, 140, blank=28)
    old = ctc_forced_align(lp, [tg], blank=28)
    assert old.feasible[0]
    old = AL.HostAlignment(old.scores[0], old.paths[0], old.starts[0], old.ends[0], True)
    assert AL.LONG_PLAN in AL.LONG_CANDIDATES
    for plan in AL.LONG_CANDIDATES + [None]:
        assert R.same(_row(ctc_forced_align_long(lp, tg, blank=28, plan=plan)), old), plan
    assert R.same(old, viterbi_align_host(lp, tg, blank=28, dtype=np.float32))


# ------------------------------------------------------------------------------------------- beyond w2l_ctc_align's limits
@pytest.mark.parametrize('t,s', [(33000, 100), (6000, 4200)])
def test_default_plan_beyond_each_old_limit(t, s):
    rng = np.random.default_rng(t)
    lp = R.log_probs(rng, t, 29)
    tg = R.target(rng, 29, s, p_repeat=0.2)
    with pytest.raises(ValueError, match='out of range'):
        ctc_forced_align(lp, [tg])
    ref = _check(lp, tg, None)
    assert ref.feasible


def test_c_entry_refuses_what_the_query_refuses():
    import ctypes as C
    from wav2letter_pytorch_amd import _lib
    x = torch.zeros(8, 4, device='cuda')
    buf = torch.zeros(4096, dtype=torch.uint8, device='cuda')
    vp = C.c_void_p
    b = vp(buf.data_ptr())
    for tb, sb, ws, what in ((24, 64, 4096, b'out of range'), (16, 0, 4096, b'out of range'), (16, 64, 64, b'needed')):
        rc = _lib.lib.w2l_ctc_align_long(vp(x.data_ptr()), 8, 4, b, 2, 0, 1, tb, sb, b, ws, b, b, b, b, b, _lib.stream_ptr())
        assert rc != 0 and what in _lib.lib.w2l_last_error(), (tb, sb, ws)
    torch.cuda.synchronize()


# -------------------------------------------------------------------------------------------------------------- the decoder
def test_decoder_align_long_equals_align():
    from wav2letter_pytorch_amd.data.label_sets import english_labels
    from wav2letter_pytorch_amd.decoder import GreedyDecoder
    labels = list(english_labels)
    dec = GreedyDecoder(labels)
    rng = np.random.default_rng(3)
    p = np.exp(R.log_probs(rng, 400, len(labels))).astype(np.float32)
    text = 'THE QUICK BROWN FOX JUMPS OVER THE LAZY DOG AA BB  CC' * 2
    offs, ends = dec.align(p, text)
    offs2, ends2 = dec.align_long(p, text)
    assert torch.equal(offs[0][0], offs2[0][0]) and torch.equal(ends[0][0], ends2[0][0]) and len(offs2[0][0]) == len(text)
    with pytest.raises(ValueError, match='no frame path'):
        dec.align_long(p[:50], text)


# ---------------------------------------------------------------------------------------------------------------- the model
def _speechlike(seed, bursts, seconds, rate=16000):
    g = np.random.default_rng(seed)
    x = 1e-3 * g.standard_normal(int(seconds * rate))
    for a, b in bursts:
        i, j = int(a * rate), int(b * rate)
        x[i:j] += 0.3 * g.standard_normal(j - i)
    return x.astype(np.float32)


@pytest.fixture(scope='module')
def model():
    from wav2letter_pytorch_amd import Wav2Letter
    from wav2letter_pytorch_amd.defaults import wav2letter_model
    torch.manual_seed(7)
    return Wav2Letter(wav2letter_model(mid_layers=1, dropout=False)).cuda().eval()


def test_align_transcript_on_a_recording_of_three_pieces(model, monkeypatch):
    from wav2letter_pytorch_amd import segmentation as SG
    from wav2letter_pytorch_amd.evaluate import frame_seconds
    monkeypatch.setattr('wav2letter_pytorch_amd.data.data_loader.SpectrogramExtractor.dithering', 0.0)
    x = _speechlike(1, ((0.5, 1.5), (2.5, 3.3), (4.2, 5.4)), 6.0)
    lines = ['the  cat sat', 'on a', 'mat']
    got = model.align_transcript(x, lines, batch_size=2)

    # the same from its parts: the pieces' posterior rows collected here, one ctc_forced_align_long, the host mapping
    rows = []

    def handle(batch, segs, out, out_lens):
        return [{'start': int(segs[i, 0]), 'end': int(segs[i, 1]), 'rows': out[j, :int(out_lens[j])].float().cpu().numpy()}
                for j, i in enumerate(batch)]

    pieces = SG.for_each_piece(model, [x], 20.0, 2, None, handle, lambda pieces, rate: sorted(pieces, key=lambda p: p['start']))[0]
    assert len(pieces) == 3
    table, at = [], 0
    for p in pieces:
        table.append((p['start'], at))
        at += p['rows'].shape[0]
        rows.append(p['rows'])
    post = np.concatenate(rows, 0)
    joined, spans = SG.transcript_lines(lines)
    assert joined == 'the cat sat on a mat'
    log_probs = bool(getattr(model, 'infer_log_probs', True))
    res = ctc_forced_align_long(post, joined, blank=int(model.ctc_decoder.blank_index), log_probs=log_probs, labels=list(model.labels))
    assert res.feasible[0]
    picked = post[np.arange(post.shape[0]), res.paths[0]]
    picked = picked if log_probs else np.log(picked)
    want = SG.alignment_records(joined, spans, res.starts[0], res.ends[0], picked, table, 16000, frame_seconds(model))
    assert [w['word'] for w in got['words']] == joined.split() and [s['text'] for s in got['segments']] == ['the cat sat', 'on a', 'mat']
    for a, b in zip(got['words'] + got['segments'], want['words'] + want['segments']):
        assert a['start'] == b['start'] and a['end'] == b['end']
        assert a['score'] == pytest.approx(b['score'], rel=1e-5, abs=1e-6)     # one log per frame: torch's on the device, numpy's here
    assert got['score'] == float(res.scores[0])
    times = [v for w in got['words'] for v in (w['start'], w['end'])]
    assert times == sorted(times) and all(w['score'] <= 0 for w in got['words'])
    # every word lies inside the sample range of the piece(s) its frames came from
    first = np.array([f for _, f in table])
    for w, (_, c0, c1) in zip(got['words'], SG.word_spans(joined)):
        p0 = int(np.searchsorted(first, res.starts[0][c0], side='right')) - 1
        p1 = int(np.searchsorted(first, res.ends[0][c1 - 1], side='right')) - 1
        assert pieces[p0]['start'] / 16000.0 <= w['start'] <= w['end']
        assert pieces[p1]['start'] / 16000.0 <= w['end'] <= pieces[p1]['end'] / 16000.0 + frame_seconds(model)
        assert w['start'] <= pieces[p0]['end'] / 16000.0 + frame_seconds(model)
    with pytest.raises(ValueError, match="'é'"):
        model.align_transcript(x, 'café')
    with pytest.raises(ValueError, match='no frame path'):
        model.align_transcript(x, 'a' * 2000)
    with pytest.raises(ValueError, match='no frame path'):
        model.align_transcript(np.zeros(32000, dtype=np.float32), 'the cat')


def test_align_transcript_under_asg_is_refused():
    from asg_replay_worker import build_model
    asg = build_model(seed=6).cuda().eval()
    with pytest.raises(NotImplementedError):
        asg.align_transcript(_speechlike(4, ((0.4, 1.2),), 2.0), 'the')
