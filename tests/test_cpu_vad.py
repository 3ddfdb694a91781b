"""Host side of long-form transcription, no GPU: the numpy restatement of the segmentation rule (tests/vad_refs.py) against
answers derived by hand (tests/vad_cases.py), the invariants of the forced split, planted defects in the reference, VadConfig's
conversions and errors, the ``transcribe`` command's argument parsing, and the stitching arithmetic."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vad_cases as VC  # noqa: E402
import vad_refs as R  # noqa: E402


@pytest.mark.parametrize('name', sorted(VC.CASES))
def test_reference_gives_the_hand_derived_segments(name):
    c = VC.CASES[name]
    got = R.segment(c['P'], **c['kw'])
    assert got['segments'].tolist() == c['want'].tolist()
    assert got['count'] == len(c['want']) and got['status'] == 0


def test_reference_statistics_and_adaptive_thresholds():
    # P = 4 1 3 2: sorted 1 2 3 4.  q = 0 -> k = 0 -> 1;  q = 1 -> k = 3 -> 4;  q = 0.5 -> k = floor(1.5) = 1 -> 2.  peak 4
    P = np.asarray([4, 1, 3, 2], dtype=np.float32)
    assert [float(R.statistics(P, q)[0]) for q in (0.0, 1.0, 0.5)] == [1.0, 4.0, 2.0]
    assert float(R.statistics(P, 0.0)[1]) == 4.0
    a = VC.ADAPTIVE
    got = R.segment(a['P'], **a['kw'])
    assert float(got['floor']) == a['floor'] and float(got['peak']) == a['peak']
    assert got['thr_on'] == a['thr_on'] and got['thr_off'] == a['thr_off']
    assert got['segments'].tolist() == a['want'].tolist()
    # the floor term wins when the floor is far below the peak: floor 1e-6, peak 1: min(1e-5, 1e-3) = 1e-5
    on, off = R.thresholds(np.float32(1e-6), np.float32(1.0), 10.0, 0.5, 1e-10)
    assert on == float(np.float32(1e-6)) * 10.0 and off == on * 0.5
    # silence: floor = peak = 0 -> abs_min
    assert R.thresholds(np.float32(0), np.float32(0), 10.0, 0.5, 1e-10) == (1e-10, 0.5e-10)
    # NaN and negative powers read as 0 and set status bit 1; cap sets bit 0 and truncates
    got = R.segment(np.asarray([2, np.nan, -1, 2, 0.25, 2], dtype=np.float32), cap=1, min_silence=1, min_speech=1, pad=0, **VC.THR)
    assert got['status'] == 3 and got['count'] == 3 and got['segments'].tolist() == [[0, 1]]


def test_frame_power_by_hand():
    # win 4, hop 2, n = 5: F = 3.  frames [0,4) [2,5) [4,5): sums 1+4+9+16 = 30, 9+16+25 = 50, 25; all divided by win = 4
    x = np.asarray([1, 2, 3, 4, 5], dtype=np.float32)
    assert R.frame_power(x, 4, 2).tolist() == [7.5, 12.5, 6.25]
    assert R.frame_power(x, 4, 2, defect='partial_own_len').tolist() == [7.5, 50 / 3, 25.0] or \
        np.allclose(R.frame_power(x, 4, 2, defect='partial_own_len'), [7.5, 50 / 3, 25.0])
    assert R.frame_power(x[:1], 4, 2).tolist() == [0.25]
    assert R.to_samples([[0, 3]], 2, 5).tolist() == [[0, 5]] and R.to_samples([[1, 2]], 2, 5).tolist() == [[2, 4]]


def test_forced_split_invariants_on_random_runs():
    rng = np.random.default_rng(7)
    for _ in range(300):
        max_frames = int(rng.integers(2, 40))
        h = max_frames // 2
        F = int(rng.integers(1, 400))
        P = rng.integers(0, 4, size=F).astype(np.float32)             # few values: equal minima are common
        a = int(rng.integers(0, F))
        b = int(rng.integers(a + 1, F + 1))
        pieces = R.forced_split([(a, b)], P, max_frames)
        assert pieces[0][0] == a and pieces[-1][1] == b
        assert all(p[1] == n[0] for p, n in zip(pieces, pieces[1:]))
        if b - a <= max_frames:
            assert pieces == [(a, b)]
        else:
            assert all(h <= e - s <= max_frames for s, e in pieces), (pieces, max_frames)
            for (s, c), _ in zip(pieces, pieces[1:]):                 # every cut is the first minimum of its window
                lo, hi = s + h, min(s + max_frames, b - h)
                assert lo <= c < hi and P[c] == P[lo:hi].min() and not (P[lo:c] == P[c]).any()


def test_planted_defects_change_an_input_the_gpu_tests_use():
    """each wrong reading of the rule differs from the right one on a crafted case (all of which the GPU tests run) or, for the
    frame power, on the row whose last frame is partial"""
    inputs = dict(VC.CASES)
    inputs.update(VC.random_cases())
    for defect in R.DEFECTS:
        if defect == 'partial_own_len':
            x = np.random.default_rng(0).standard_normal(3 * 160 + 37).astype(np.float32)
            assert not np.array_equal(R.frame_power(x, 320, 160), R.frame_power(x, 320, 160, defect=defect))
            continue
        hit = [n for n, c in inputs.items()
               if R.segment(c['P'], defect=defect, **c['kw'])['segments'].tolist() != R.segment(c['P'], **c['kw'])['segments'].tolist()]
        assert hit, defect
    # and the crafted case aimed at each one catches it
    aimed = dict(on_gt='ties', off_le='ties', close_drop_swap='close_then_drop', gap_off_by_one='gap', last_min='split_ties',
                 carry_1024='carry')
    for defect, name in aimed.items():
        c = VC.CASES[name]
        assert R.segment(c['P'], defect=defect, **c['kw'])['segments'].tolist() != c['want'].tolist(), defect


def test_vad_config_conversions_and_errors():
    from wav2letter_pytorch_amd.segmentation import VadConfig
    cfg = VadConfig()
    assert (cfg.win, cfg.hop, cfg.n_fft) == (320, 160, 512)
    n = cfg.numbers(20.0)
    assert (n['min_silence'], n['min_speech'], n['pad'], n['max_frames'], n['absolute']) == (30, 10, 20, 2000, 0)
    assert n['r_on'] == 10.0 ** (10.0 / 10.0) and n['r_hyst'] == 10.0 ** (-3.0 / 10.0) and n['q'] == 0.05 and n['abs_min'] == 1e-10
    assert cfg.numbers(15.0)['max_frames'] == 1500 and cfg.numbers(0.065)['max_frames'] == 6       # floor(6.5)
    ab = VadConfig(on_dbfs=-40.0)
    n = ab.numbers()
    assert n['absolute'] == 1 and n['thr_on'] == 10.0 ** -4.0 and n['thr_off'] == 10.0 ** (-43.0 / 10.0)
    assert VadConfig(on_dbfs=-40, off_dbfs=-46).numbers()['thr_off'] == 10.0 ** -4.6
    other = VadConfig.for_model(dict(sample_rate=8000, window_size=0.032, window_stride=0.016, window='hamming'))
    assert (other.win, other.hop, other.n_fft, other.frames(0.3)) == (256, 128, 256, 19)
    # the shortest segment: min_speech frames with a partial last one, (frames - 1) hop + 1 samples, must exceed n_fft / 2 = 256
    assert VadConfig(min_speech=0.03).shortest_samples(3) == 321
    for bad in (dict(min_speech=0.02), dict(min_speech=0.0), dict(q=1.5), dict(q=-0.1), dict(hyst_db=-1), dict(on_db=float('nan')),
                dict(off_dbfs=-50), dict(on_dbfs=-50, off_dbfs=-40), dict(pad=-0.1), dict(window_stride=0.03)):
        with pytest.raises(ValueError):
            VadConfig(**bad)
    for bad in (0.01, 0.03):                             # 1 and 3 frames: below 2 frames, and pieces of h = 1 frame
        with pytest.raises(ValueError):
            cfg.numbers(bad)
    from wav2letter_pytorch_amd.segmentation import vad_params
    p = vad_params(cfg.numbers(20.0))
    assert (p.max_frames, p.min_silence, p.absolute, p.r_on) == (2000, 30, 0, 10.0)


def test_parse_records_layout():
    from wav2letter_pytorch_amd.segmentation import HEADER_BYTES, parse_records
    cap = 3
    buf = np.zeros(2 * (HEADER_BYTES + 8 * cap), dtype=np.uint8)
    for i, (count, status) in enumerate(((2, 0), (5, 1))):
        rec = buf[i * (HEADER_BYTES + 8 * cap):]
        rec[:8].view(np.int32)[:] = (count, status)
        rec[8:24].view(np.float64)[:] = (0.5 + i, 0.25 + i)
        rec[24:32].view(np.float32)[:] = (0.125, 4.0)
        rec[HEADER_BYTES: HEADER_BYTES + 8 * cap].view(np.int32)[:] = np.arange(6) + 10 * i
    a, b = parse_records(buf, 2, cap)
    assert (a['count'], a['status'], a['thr_on'], a['thr_off'], float(a['floor']), float(a['peak'])) == (2, 0, 0.5, 0.25, 0.125, 4.0)
    assert a['frames'].tolist() == [[0, 1], [2, 3]]
    assert (b['count'], b['status'], b['thr_on']) == (5, 1, 1.5) and b['frames'].tolist() == [[10, 11], [12, 13], [14, 15]]


def test_transcribe_command_argument_parsing():
    from wav2letter_pytorch_amd import transcribe as TR
    cfg = TR.build_config(['model_path=m.ckpt', 'audio=a.wav,b.wav', 'segment.max_seconds=15', 'segment.on_db=8', 'word_times=true',
                           'decoder=beam', 'beam.k=3', 'batch_size=2', 'output=o.jsonl', 'model.mid_layers=2'])
    assert cfg.audio == ['a.wav', 'b.wav'] and dict(cfg.segment) == {'max_seconds': 15.0, 'on_db': 8.0}
    assert (cfg.batch_size, cfg.word_times, cfg.decoder, cfg.beam.k, cfg.output, cfg.model.mid_layers) == (2, True, 'beam', 3, 'o.jsonl', 2)
    vad = TR.vad_config(cfg)
    assert vad.on_db == 8.0 and vad.hyst_db == 3.0 and vad.numbers(cfg.segment.max_seconds)['max_frames'] == 1500
    cfg = TR.build_config(['model_path=m.ckpt', 'audio=one.wav'])
    assert cfg.audio == ['one.wav'] and cfg.batch_size == 8 and cfg.segment.max_seconds == 20.0 and cfg.decoder == 'greedy'
    assert not cfg.word_times and cfg.output is None
    from wav2letter_pytorch_amd import test as T
    assert T.decoder_spec(TR.build_config(['model_path=m', 'audio=a.wav', 'decoder=beam', 'beam.k=7']), True)[1]['k'] == 7
    for bad in (['audio=a.wav'], ['model_path=m.ckpt'], ['model_path=m', 'audio=a.wav', 'segment.nope=1'],
                ['model_path=m', 'audio=a.wav', 'segment.pad=soon'], ['model_path=m', 'audio=a.wav', 'batch_size=0'],
                ['model_path=m', 'audio=a.wav', 'decoder=beam_lm'], ['model_path=m', 'audio=a.wav', 'lm_path=x.arpa']):
        with pytest.raises(SystemExit):
            TR.build_config(bad)
    with pytest.raises(ValueError):
        TR.vad_config(TR.build_config(['model_path=m', 'audio=a.wav', 'segment.min_speech=0.01']))


def test_stitching_offsets_and_word_times():
    from wav2letter_pytorch_amd.segmentation import batches_by_length, stitch
    pieces = [  # out of time order, as length-sorted batches return them
        dict(start=48000, end=80000, text='c d', words=[('c', 0.25, 0.5), ('d', 1.0, 1.5)]),
        dict(start=8000, end=24000, text='a b', words=[('a', 0.0, 0.125), ('b', 0.5, 0.75)]),
        dict(start=32000, end=40000, text='', words=[]),
    ]
    got = stitch(pieces, 16000, word_times=True)
    assert got['text'] == 'a b c d'
    assert [(s['start'], s['end'], s['text']) for s in got['segments']] == [(0.5, 1.5, 'a b'), (2.0, 2.5, ''), (3.0, 5.0, 'c d')]
    assert got['segments'][0]['words'] == [{'word': 'a', 'start': 0.5, 'end': 0.625}, {'word': 'b', 'start': 1.0, 'end': 1.25}]
    assert got['segments'][2]['words'] == [{'word': 'c', 'start': 3.25, 'end': 3.5}, {'word': 'd', 'start': 4.0, 'end': 4.5}]
    assert got['segments'][1]['words'] == []
    plain = stitch(pieces, 16000)
    assert all('words' not in s for s in plain['segments']) and plain['text'] == 'a b c d'
    assert stitch([], 16000, word_times=True) == {'text': '', 'segments': []}
    assert batches_by_length([5, 9, 7, 9, 1], 2) == [[1, 3], [2, 0], [4]]
    assert batches_by_length([], 4) == []


def test_transcribe_long_is_part_of_the_model_surface():
    import inspect
    from wav2letter_pytorch_amd.base_asr_models import ConvCTCASR
    from wav2letter_pytorch_amd.data.data_loader import SpectrogramExtractor
    sig = inspect.signature(ConvCTCASR.transcribe_long).parameters
    assert list(sig)[1:] == ['items', 'max_seconds', 'batch_size', 'decoder', 'word_times', 'vad']
    assert (sig['max_seconds'].default, sig['batch_size'].default, sig['word_times'].default) == (20.0, 8, False)
    assert 'batch_size=1' in ConvCTCASR.transcribe_long.__doc__
    assert list(inspect.signature(SpectrogramExtractor.extract_rows).parameters)[1:] == ['audio', 'lens', 'noise']
    assert math.isclose(VC.ADAPTIVE['thr_on'] ** 2, 0.5)
