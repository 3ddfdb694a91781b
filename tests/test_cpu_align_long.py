"""The host side of the long alignment (csrc/ctc_align_long.hip, alignment.ctc_forced_align_long, segmentation.align_transcript,
align.py), without a GPU: the tiled scheme emulated in NumPy (tests/align_long_refs.py) is bit-equal to
alignment.viterbi_align_host in float32 on the device cases' inputs, every planted defect changes a result there, and the
workspace query, the exported symbols, the argument errors, the clock table and the line bookkeeping are what they say."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import align_long_refs as R  # noqa: E402

from wav2letter_pytorch_amd import alignment as AL  # noqa: E402
from wav2letter_pytorch_amd import segmentation as SG  # noqa: E402
from wav2letter_pytorch_amd.alignment import viterbi_align_host  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _runs():
    """(name, lp, target, plan) over every small device case"""
    for name, lp, tg in R.grid_cases():
        for plan in R.SMALL_PLANS:
            yield name, lp, tg, plan
    for name, lp, tg in R.single_path_cases():
        for plan in R.SINGLE_PLANS:
            yield name, lp, tg, plan


@pytest.fixture(scope='module')
def refs():
    return {name: viterbi_align_host(lp, tg, dtype=np.float32) for name, lp, tg in R.grid_cases() + R.single_path_cases()}


def test_emulation_is_bit_equal_to_the_host_model(refs):
    feasible = 0
    for name, lp, tg, (tb, sb) in _runs():
        for halo in (None, 2 * tb):                      # the kernel's window, and the least the argument allows
            got = R.tiled_align(lp, tg, 0, tb, sb, halo=halo)
            assert R.same(got, refs[name]), (name, tb, sb, halo)
        feasible += bool(refs[name].feasible)
    assert feasible >= 30
    assert refs['single T=S'].feasible and not refs['single T=S-1'].feasible
    assert refs['single T=S+repeats'].feasible and not refs['single T=S+repeats-1'].feasible
    assert refs['single T=S'].starts.tolist() == list(range(100))
    assert refs['single staircase+31'].starts.tolist() == [0] + list(range(32, 131))


def test_emulation_other_blank_and_planner_shapes():
    rng = np.random.default_rng(5)
    lp = R.log_probs(rng, 300, 29, holes=0.03)
    tg = R.target(rng, 29, 140, blank=28)
    ref = viterbi_align_host(lp, tg, blank=28, dtype=np.float32)
    assert ref.feasible
    for tb, sb in AL.LONG_CANDIDATES:
        assert R.same(R.tiled_align(lp, tg, 28, tb, sb), ref), (tb, sb)


@pytest.mark.parametrize('defect', R.DEFECTS)
def test_planted_defect_changes_a_device_case(defect, refs):
    caught = [(name, plan) for name, lp, tg, plan in _runs()
              if not R.same(R.tiled_align(lp, tg, 0, plan[0], plan[1], halo=2 * plan[0], defect=defect), refs[name])]
    print(defect, 'caught by', caught)
    assert caught, defect
    if defect == 'short_halo':
        # only the path that climbs two states per frame from just below a window reaches the halo's top: the T = S staircase
        # at an odd offset from the tiles, under the plans whose halo is exactly 2 tb
        assert {name for name, _ in caught} == {'single staircase+31'} and ('single staircase+31', (32, 64)) in caught


def test_short_halo_hides_from_random_posteriors():
    """why the single-path case is kept: with room to spare (T = 4 S) the best path never runs along the cone's edge"""
    rng = np.random.default_rng(9)
    lp = R.log_probs(rng, 280, 29)
    tg = R.target(rng, 29, 70)
    ref = viterbi_align_host(lp, tg, dtype=np.float32)
    assert R.same(R.tiled_align(lp, tg, 0, 16, 64, defect='short_halo'), ref)


# ------------------------------------------------------------------------------------------------------------- the C surface
def test_workspace_bytes_formula_and_refusals():
    from wav2letter_pytorch_amd._lib import lib
    q = lib.w2l_ctc_align_long_workspace_bytes
    for t, s, tb, sb in [(1, 0, 16, 64), (70, 100, 16, 64), (70, 100, 48, 2048), (33000, 100, 64, 384), (180000, 50000, 256, 1536),
                         (1 << 22, 1 << 20, 16, 64)]:
        lpad = -(-(2 * s + 1) // sb) * sb
        want = 16 + 2 * lpad * 4 + -(-t * 4 // 16) * 16 + -(-t // 16) * lpad * 4
        assert q(t, s, tb, sb) == want == AL.long_workspace_bytes(t, s, tb, sb), (t, s, tb, sb)
    assert q(180000, 50000, 64, 384) // 10 ** 8 == 45                       # "about 4.5 GB for one hour"
    assert q(300, 140, 0, 0) == AL.long_workspace_bytes(300, 140, *AL.LONG_PLAN)
    assert AL.LONG_PLAN in AL.LONG_CANDIDATES
    for bad in [(0, 5, 0, 0), ((1 << 22) + 1, 5, 0, 0), (10, -1, 0, 0), (10, (1 << 20) + 1, 0, 0),       # out of range
                (10, 5, 16, 0), (10, 5, 0, 64), (10, 5, 8, 64), (10, 5, 24, 64), (10, 5, 272, 64), (10, 5, -16, 64),
                (10, 5, 16, 32), (10, 5, 16, 96), (10, 5, 16, 2112), (10, 5, 16, -64)]:                   # invalid forced plans
        assert q(*bad) == -1, bad


def test_header_and_exports_agree():
    from wav2letter_pytorch_amd import _lib
    text = open(os.path.join(ROOT, 'include', 'w2l_hip.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    for name in ('w2l_ctc_align_long_workspace_bytes', 'w2l_ctc_align_long'):
        assert re.search(r'\b%s\s*\(' % name, text) and name in _lib.EXPORTED_SYMBOLS and hasattr(_lib.lib, name)
    args = re.search(r'int w2l_ctc_align_long\((.*?)\);', text, flags=re.S).group(1)
    assert len(args.split(',')) == len(_lib._SIGNATURES['w2l_ctc_align_long'][1]) == 17
    for macro, value in (('MAX_T', AL.LONG_MAX_T), ('MAX_S', AL.LONG_MAX_S), ('MAX_TB', AL.LONG_MAX_TB), ('MAX_SB', AL.LONG_MAX_SB),
                         ('TB', AL.LONG_PLAN[0]), ('SB', AL.LONG_PLAN[1])):
        got = re.search(r'#define W2L_ALIGN_LONG_%s\s+(\(?[0-9 <]+\)?)' % macro, text).group(1)
        assert eval(got) == value, macro
    assert _lib.lib.w2l_abi_version() == 2


def test_argument_errors_come_before_the_device():
    lp = np.zeros((20, 5), dtype=np.float32)
    f = AL.ctc_forced_align_long
    for kw, match in [(dict(probs=np.zeros((2, 20, 5), dtype=np.float32), target=[1]), 'one recording'),
                      (dict(probs=np.zeros((0, 5), dtype=np.float32), target=[1]), 'empty'),
                      (dict(probs=lp, target=[1], blank=5), 'blank'),
                      (dict(probs=lp, target=[1], labels=list('abc')), 'labels'),
                      (dict(probs=lp, target='ab'), 'labels'),
                      (dict(probs=lp, target='az', labels=list('_abcd')), "'z'"),
                      (dict(probs=lp, target=[[1, 2], [3, 4]]), 'ONE sequence'),
                      (dict(probs=lp, target=[1.5]), 'integers'),
                      (dict(probs=lp, target=[1], plan=(16,)), 'pair'),
                      (dict(probs=lp, target=[1], plan=(24, 64)), 'multiple of 16'),
                      (dict(probs=lp, target=[1], plan=(16, 100)), 'multiple of 64'),
                      (dict(probs=lp, target=[1], plan=(512, 64)), 'multiple of 16'),
                      (dict(probs=lp, target=np.ones((1 << 20) + 1, dtype=np.int32)), 'out of range')]:
        with pytest.raises(ValueError, match=match):
            f(**kw)


def test_workspace_above_the_cap_is_refused_with_its_size():
    import torch
    t, s = 180000, 50000
    need = AL.long_workspace_bytes(t, s, *AL.LONG_PLAN)
    assert need > 4 << 30
    probs = torch.zeros(1, 29).expand(t, 29)               # [T, A] without its memory
    with pytest.raises(ValueError, match=str(need)):
        AL.ctc_forced_align_long(probs, np.ones(s, dtype=np.int32), max_workspace_bytes=4 << 30)
    with pytest.raises(ValueError, match=str(AL.long_workspace_bytes(20, 3, 16, 64))):
        AL.ctc_forced_align_long(np.zeros((20, 5), dtype=np.float32), [1, 2, 3], plan=(16, 64), max_workspace_bytes=100)


# --------------------------------------------------------------------------------------------------- clock and bookkeeping
def test_transcript_lines_and_word_spans():
    joined, spans = SG.transcript_lines(['  the  cat\tsat ', 'on\nthe mat'])
    assert joined == 'the cat sat on the mat'
    assert [joined[a:b] for a, b in spans] == ['the cat sat', 'on the mat']
    assert SG.transcript_lines(' a  b ') == ('a b', [(0, 3)])
    assert [(w, joined[a:b]) for w, a, b in SG.word_spans(joined)] == [(w, w) for w in joined.split()]
    for bad in ([], ['a', '  '], [''], ['a', 3]):
        with pytest.raises(ValueError):
            SG.transcript_lines(bad)


def test_frame_times_across_pieces():
    table = [(1600, 0), (48000, 10), (80000, 25)]         # pieces at 0.1 s, 3.0 s and 5.0 s with 10, 15 and more frames
    got = SG.frame_times([0, 9, 10, 24, 25, 30], table, 16000, 0.02)
    assert np.allclose(got, [0.1, 0.1 + 9 * 0.02, 3.0, 3.0 + 14 * 0.02, 5.0, 5.0 + 5 * 0.02], rtol=0, atol=1e-12)
    for bad in ([], [(0, 1)], [(0, 0), (5, 0)]):
        with pytest.raises(ValueError):
            SG.frame_times([0], bad, 16000, 0.02)
    with pytest.raises(ValueError):
        SG.frame_times([-1], table, 16000, 0.02)


def test_alignment_records_with_a_word_across_two_pieces():
    joined, spans = SG.transcript_lines(['ab cd', 'e'])
    #            a  b ' ' c   d  ' '  e
    starts = [1, 3, 5, 8, 11, 13, 14]
    ends = [2, 4, 6, 9, 12, 13, 16]
    table = [(1600, 0), (48000, 10)]                       # "cd" starts in piece 0 (frame 8) and ends in piece 1 (frame 12)
    logp = -np.arange(18, dtype=np.float64)
    got = SG.alignment_records(joined, spans, starts, ends, logp, table, 16000, 0.02)
    words = got['words']
    assert [w['word'] for w in words] == ['ab', 'cd', 'e']
    assert words[0]['start'] == pytest.approx(0.1 + 1 * 0.02) and words[0]['end'] == pytest.approx(0.1 + 4 * 0.02)
    assert words[1]['start'] == pytest.approx(0.1 + 8 * 0.02) and words[1]['end'] == pytest.approx(3.0 + 2 * 0.02)
    assert words[1]['score'] == pytest.approx(-np.mean([8, 9, 10, 11, 12]))
    assert words[2]['score'] == pytest.approx(-15.0)
    segs = got['segments']
    assert [s['text'] for s in segs] == ['ab cd', 'e']
    assert segs[0]['start'] == words[0]['start'] and segs[0]['end'] == words[1]['end']
    assert segs[0]['score'] == pytest.approx(-np.mean(np.arange(1, 13)))
    assert {k: segs[1][k] for k in ('start', 'end', 'score')} == {k: words[2][k] for k in ('start', 'end', 'score')}
    assert got['score'] == pytest.approx(logp.sum())
    times = [v for w in words for v in (w['start'], w['end'])]
    assert times == sorted(times)


def test_align_build_config_and_segment_words():
    from wav2letter_pytorch_amd import align as A
    cfg = A.build_config(['model_path=m.ckpt', 'audio=a.wav', 'text=a.txt', 'segment.max_seconds=12', 'batch_size=2'])
    assert cfg.audio == ['a.wav'] and str(cfg.text) == 'a.txt' and cfg.segment.max_seconds == 12.0 and cfg.batch_size == 2
    for bad in (['model_path=m.ckpt', 'audio=a.wav'], ['model_path=m.ckpt', 'audio=a.wav,b.wav', 'text=a.txt'],
                ['model_path=m.ckpt', 'text=a.txt'], ['model_path=m.ckpt', 'audio=a.wav', 'text=a.txt', 'model.criterion=asg'],
                ['model_path=m.ckpt', 'audio=a.wav', 'text=a.txt', 'segment.nope=1']):
        with pytest.raises(SystemExit):
            A.build_config(bad)
    result = {'words': [{'word': w} for w in 'the cat sat on mat'.split()], 'segments': [{'text': 'the cat sat'}, {'text': 'on mat'}]}
    got = A.segment_words(result)
    assert [[w['word'] for w in s['words']] for s in got] == [['the', 'cat', 'sat'], ['on', 'mat']]


def test_read_lines(tmp_path):
    from wav2letter_pytorch_amd import align as A
    p = tmp_path / 'a.txt'
    p.write_text('the  cat\n\n  sat \n')
    assert A.read_lines(str(p)) == ['the cat', 'sat']
    p.write_text('\n \n')
    with pytest.raises(SystemExit):
        A.read_lines(str(p))
    with pytest.raises(SystemExit):
        A.read_lines(str(tmp_path / 'none.txt'))
