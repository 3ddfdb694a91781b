"""Long-form transcription on a real MI355X: w2l_vad_power and w2l_vad_segments through the C ABI against the numpy
restatement of the rule (tests/vad_refs.py) and the hand-derived answers (tests/vad_cases.py), segmentation.vad_segments from
the waveform, ConvCTCASR.transcribe_long against transcribe of the same slices, and the transcribe command line."""
import ctypes as C
import json
import os
import sys
import wave

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vad_cases as VC  # noqa: E402
import vad_refs as R  # noqa: E402

pytestmark = pytest.mark.gpu

WIN, HOP = 320, 160
ULP64 = 2.0 ** -53


def _numbers(kw):
    """the parameter dict of a case (vad_refs.segment keywords) -> the fields of w2l_vad_params_t"""
    n = dict(q=0.05, r_on=10.0, r_hyst=0.5, abs_min=1e-10, thr_on=0.0, thr_off=0.0, absolute=0, min_silence=1, min_speech=1, pad=0,
             max_frames=100000)
    n.update(kw)
    n['absolute'] = int('thr_on' in kw)
    return n


def _decide(P_rows, kw, cap=256, grow=True, stride=None):
    """power arrays (one per recording) -> the device's records, through one launch"""
    from wav2letter_pytorch_amd.segmentation import segments_from_power
    stride = stride or max(1, max(len(p) for p in P_rows))
    host = np.full((len(P_rows), stride), 9.0, dtype=np.float32)          # beyond a row's frames: speech-level powers it must not read
    for i, p in enumerate(P_rows):
        host[i, :len(p)] = p
    power = torch.from_numpy(host).cuda()
    nfr = torch.tensor([len(p) for p in P_rows], dtype=torch.int32).cuda()
    return segments_from_power(power, nfr, _numbers(kw), cap=cap, grow=grow)


def _same_as_reference(rec, P, kw, cap=None):
    """the device's record against the reference run on the same powers and the device's own thresholds"""
    ref_kw = dict(kw)
    ref_kw.update(thr_on=rec['thr_on'], thr_off=rec['thr_off'])
    want = R.segment(P, cap=cap, **ref_kw)
    assert rec['count'] == want['count'] and rec['status'] == want['status'], (rec['count'], want['count'], rec['status'])
    assert rec['frames'].tolist() == want['segments'].tolist()
    floor, peak = R.statistics(P, kw.get('q', 0.05))
    assert rec['floor'] == floor and rec['peak'] == peak


def test_frame_power_against_the_reference_and_bit_reproducible():
    from wav2letter_pytorch_amd.segmentation import frame_power
    g = np.random.default_rng(3)
    lens = [5 * 1024 * HOP + 37, WIN - 1, 4000]
    L = (max(lens) + 3) // 4 * 4                         # rows on 16-byte boundaries: the vector loads
    x = np.full((3, L), 3.0, dtype=np.float32)           # beyond a row's length: NOT zero -- the kernel must not read it
    x[0, :lens[0]] = (0.3 * g.standard_normal(lens[0])).astype(np.float32)
    x[1, :lens[1]] = (0.3 * g.standard_normal(lens[1])).astype(np.float32)
    x[2, :lens[2]] = 0.0
    nfr = [-(-n // HOP) for n in lens]
    fmax = max(nfr) + 3                                  # frames past a row's own are written as zeros
    xd, ld = torch.from_numpy(x).cuda(), torch.tensor(lens, dtype=torch.int32).cuda()
    got = frame_power(xd, ld, fmax, WIN, HOP).cpu().numpy()
    again = frame_power(xd, ld, fmax, WIN, HOP).cpu().numpy()
    assert np.array_equal(got.view(np.uint32), again.view(np.uint32))
    tol = (WIN + 2) * ULP64

    def check(got_row, samples):
        sums, _ = R.frame_sums(samples, WIN, HOP)
        v = sums / WIN
        lo, hi = (v * (1 - tol)).astype(np.float32), (v * (1 + tol)).astype(np.float32)
        F = len(v)
        bad = np.nonzero((got_row[:F] < lo) | (got_row[:F] > hi))[0]
        assert bad.size == 0, (bad[:5], got_row[bad[:5]], v[bad[:5]])
        assert not got_row[F:].any()
        ref = R.frame_power(samples, WIN, HOP)
        print(f'frames {F}: {int((got_row[:F] != ref).sum())} differ from the sequential sum by an fp32 ulp')

    for i, n in enumerate(lens):
        check(got[i], x[i, :n])
    assert not got[2].any()
    # an odd row stride and an unaligned base: the scalar loads
    odd = torch.from_numpy(np.ascontiguousarray(x[:, :2 * 1024 * HOP + 39])).cuda()
    lens2 = [2 * 1024 * HOP + 39, WIN - 1, 777]
    got2 = frame_power(odd, torch.tensor(lens2, dtype=torch.int32).cuda(), -(-lens2[0] // HOP), WIN, HOP).cpu().numpy()
    for i, n in enumerate(lens2):
        check(got2[i], x[i, :n])
    # other frame geometries: hop == win, a window above one block's span of hops
    for win, hop in ((256, 256), (400, 160), (3000, 100), (7, 3)):
        n = 20011
        sig = (0.2 * g.standard_normal(n)).astype(np.float32)
        F = -(-n // hop)
        out = frame_power(torch.from_numpy(sig).cuda().view(1, -1), torch.tensor([n], dtype=torch.int32).cuda(), F, win, hop).cpu().numpy()[0]
        sums, _ = R.frame_sums(sig, win, hop)
        v = sums / win
        t = (win + 2) * ULP64
        assert ((out >= (v * (1 - t)).astype(np.float32)) & (out <= (v * (1 + t)).astype(np.float32))).all(), (win, hop)


@pytest.mark.parametrize('name', sorted(VC.CASES))
def test_decisions_on_crafted_powers(name):
    c = VC.CASES[name]
    rec = _decide([c['P']], c['kw'])[0]
    assert rec['frames'].tolist() == c['want'].tolist()
    assert rec['thr_on'] == 1.0 and rec['thr_off'] == 0.5
    _same_as_reference(rec, c['P'], c['kw'])


def test_decisions_batched_random_powers_every_tile_size():
    cases = VC.random_cases()
    names = sorted(cases)
    kw = cases[names[0]]['kw']
    recs = _decide([cases[n]['P'] for n in names], kw)
    for n, rec in zip(names, recs):
        _same_as_reference(rec, cases[n]['P'], kw)
    big = cases['random_5157']
    assert _decide([big['P']], kw)[0]['count'] > 20
    # the same powers in adaptive mode at several quantiles, q = 0 and q = 1 among them
    for q in (0.0, 0.05, 0.5, 1.0):
        akw = dict(q=q, r_on=3.0, r_hyst=0.5, abs_min=1e-10, min_silence=3, min_speech=4, pad=2, max_frames=24)
        for n, rec in zip(names, _decide([cases[n]['P'] for n in names], akw)):
            floor, peak = R.statistics(cases[n]['P'], q)
            assert rec['floor'] == floor and rec['peak'] == peak, (n, q)
            on, off = R.thresholds(floor, peak, 3.0, 0.5, 1e-10)
            assert abs(rec['thr_on'] - on) <= np.spacing(on) and abs(rec['thr_off'] - off) <= np.spacing(off), (n, q)
            _same_as_reference(rec, cases[n]['P'], akw)
    # many distinct values: the radix select walks all four bytes
    g = np.random.default_rng(5)
    P = (g.random(4099) ** 4).astype(np.float32)
    akw = dict(q=0.31, r_on=4.0, r_hyst=0.7, abs_min=1e-10, min_silence=2, min_speech=2, pad=1, max_frames=40)
    rec = _decide([P], akw)[0]
    _same_as_reference(rec, P, akw)


def test_adaptive_mode_by_hand_cap_and_bad_powers():
    a = VC.ADAPTIVE
    rec = _decide([a['P']], a['kw'])[0]
    assert float(rec['floor']) == a['floor'] and float(rec['peak']) == a['peak']
    assert abs(rec['thr_on'] - a['thr_on']) <= np.spacing(a['thr_on']) and abs(rec['thr_off'] - a['thr_off']) <= np.spacing(a['thr_off'])
    assert rec['frames'].tolist() == a['want'].tolist() and rec['status'] == 0
    # cap below count: the count the rule yields, bit 0, the first cap segments; growing repeats the launch
    big = VC.random_cases()['random_5157']
    full = _decide([big['P']], big['kw'])[0]
    cut = _decide([big['P']], big['kw'], cap=5, grow=False)[0]
    assert cut['count'] == full['count'] > 5 and cut['status'] == 1 and cut['frames'].tolist() == full['frames'][:5].tolist()
    _same_as_reference(cut, big['P'], big['kw'], cap=5)
    grown = _decide([big['P']], big['kw'], cap=5)[0]
    assert grown['status'] == 0 and grown['frames'].tolist() == full['frames'].tolist()
    # NaN and negative powers: read as 0, reported in bit 1
    P = np.asarray([2, np.nan, -1, 2, 0.25, 2, -0.0, 2], dtype=np.float32)
    kw = dict(VC.THR, min_silence=1, min_speech=1, pad=0, max_frames=100)
    rec = _decide([P], kw)[0]
    assert rec['status'] == 2 and rec['frames'].tolist() == [[0, 1], [3, 4], [5, 6], [7, 8]]
    _same_as_reference(rec, P, kw)
    # silence in adaptive mode: abs_min is the threshold, nothing is speech
    rec = _decide([np.zeros(700, dtype=np.float32)], a['kw'])[0]
    assert rec['count'] == 0 and rec['thr_on'] == 1e-10 and rec['floor'] == 0 and rec['peak'] == 0


def test_argument_errors_launch_nothing():
    from wav2letter_pytorch_amd._lib import W2LError, lib, ptr, stream_ptr
    from wav2letter_pytorch_amd.segmentation import vad_params
    x = torch.zeros(1, 4000, device='cuda')
    lens = torch.tensor([4000], dtype=torch.int32).cuda()
    power = torch.zeros(1, 25, device='cuda')
    assert lib.w2l_vad_power(ptr(x), 4000, ptr(lens), 1, 160, 320, ptr(power), 25, stream_ptr()) != 0          # hop > win
    assert b'hop' in lib.w2l_last_error()
    assert lib.w2l_vad_power(ptr(x), 4000, ptr(lens), 1, 320, 160, ptr(power), 24, stream_ptr()) != 0          # 25 frames needed
    assert lib.w2l_vad_power(ptr(x), 4000, ptr(lens), 1, 320, 160, ptr(power), 1 << 24, stream_ptr()) != 0
    assert lib.w2l_vad_power(ptr(x), 4000, ptr(lens), 1, 320, 160, ptr(power), 25, stream_ptr()) == 0
    ws_bytes = int(lib.w2l_vad_workspace_bytes(1, 25))
    assert ws_bytes > 0
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device='cuda')
    out = torch.full((32 + 8 * 4,), 7, dtype=torch.uint8, device='cuda')
    nfr = torch.tensor([25], dtype=torch.int32).cuda()
    good = _numbers(dict(max_frames=10))

    def call(numbers=good, cap=4, ws_bytes=ws_bytes, stride=25):
        p = vad_params(numbers)
        return lib.w2l_vad_segments(ptr(power), stride, ptr(nfr), 1, C.byref(p), cap, ptr(ws), ws_bytes, ptr(out), stream_ptr())

    for bad in (dict(max_frames=1), dict(q=1.5), dict(q=-0.1), dict(q=float('nan')), dict(r_on=float('inf')), dict(r_hyst=float('nan')),
                dict(r_hyst=1.5), dict(pad=-1)):
        assert call(dict(good, **bad)) != 0, bad
        assert lib.w2l_last_error()
    assert call(cap=0) != 0 and call(ws_bytes=ws_bytes - 1) != 0 and call(stride=1 << 24) != 0
    torch.cuda.synchronize()
    assert bool((out == 7).all())                        # nothing was launched
    assert call() == 0
    torch.cuda.synchronize()
    assert int(out[:4].view(torch.int32)[0]) == 0        # zero powers: no segments
    with pytest.raises(W2LError):
        _decide([np.zeros(10, dtype=np.float32)], dict(max_frames=1))


def test_segments_from_the_waveform_end_to_end():
    from wav2letter_pytorch_amd.segmentation import VadConfig, vad_segments
    x = VC.synthetic_recording(0, -60.0)
    cfg = VadConfig()
    numbers = cfg.numbers(15.0)
    kw = {k: numbers[k] for k in ('q', 'r_on', 'r_hyst', 'abs_min', 'min_silence', 'min_speech', 'pad', 'max_frames')}
    ref = R.vad_reference(x, WIN, HOP, **kw)
    # the input's margins, on the reference alone: if either fails the input is wrong, not the kernel
    P = ref['power'].astype(np.float64)
    for thr in (ref['thr_on'], ref['thr_off']):
        margin = np.abs(10 * np.log10(np.maximum(P, 1e-30) / thr)).min()
        print(f'margin to {thr:.3e}: {margin:.2f} dB')
        assert margin > 1.0
    h = kw['max_frames'] // 2
    runs = R.pad_merge(R.drop_short(R.close_gaps(R.runs_of(R.hysteresis(ref['power'], ref['thr_on'], ref['thr_off'])), kw['min_silence']),
                                    kw['min_speech']), kw['pad'], len(P))
    cuts = 0
    for a, b in runs:
        while b - a > kw['max_frames']:
            w = np.sort(P[a + h: min(a + kw['max_frames'], b - h)])
            assert w[1] >= 2 * w[0]
            a = a + h + int(np.argmin(P[a + h: min(a + kw['max_frames'], b - h)]))
            cuts += 1
    assert cuts == 1
    # by construction: bursts 1 and 2 joined and padded, the 50 ms burst dropped, the 19 s burst cut at the dip (frame 1604)
    assert ref['segments'].tolist() == [[79, 420], [579, 1604], [1604, 2520]]
    segs, stats = vad_segments([torch.from_numpy(x).cuda()], cfg, max_seconds=15.0, return_stats=True)
    assert stats[0]['frames'].tolist() == ref['segments'].tolist() and stats[0]['status'] == 0
    assert segs[0].dtype == np.int64 and segs[0].tolist() == ref['samples'].tolist()
    assert stats[0]['floor'] == ref['floor'] and stats[0]['peak'] == ref['peak']
    # host arrays, several recordings of different lengths at once, silence among them
    many = vad_segments([x, np.zeros(16000, dtype=np.float32), x[:7 * 16000 + 5]], cfg, max_seconds=15.0)
    assert many[0].tolist() == ref['samples'].tolist() and many[1].shape == (0, 2)
    short = R.vad_reference(x[:7 * 16000 + 5], WIN, HOP, **kw)
    assert many[2].tolist() == short['samples'].tolist() and many[2][-1, 1] == 7 * 16000 + 5


# ---------------------------------------------------------------------------------------------------------------- the model
def _speechlike(seed, bursts, seconds, rate=16000):
    """noise at -60 dBFS with bursts of louder noise: random weights give such input a non-trivial transcript"""
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


def test_transcribe_long_equals_transcribe_of_its_segments(model, monkeypatch):
    from wav2letter_pytorch_amd.data.resample import resample_batch
    from wav2letter_pytorch_amd.segmentation import vad_segments
    monkeypatch.setattr('wav2letter_pytorch_amd.data.data_loader.SpectrogramExtractor.dithering', 0.0)
    x = _speechlike(1, ((0.5, 1.5), (2.5, 3.3), (4.0, 5.5)), 6.0)
    segs = vad_segments([x])[0]
    assert len(segs) == 3
    got = model.transcribe_long([x], batch_size=1, word_times=True)[0]
    assert len(got['segments']) == 3
    texts = []
    for seg, (a, b) in zip(got['segments'], segs.tolist()):
        text, words = model.transcribe([x[a:b]], batch_size=1, word_times=True)[0]
        assert seg['text'] == text and seg['start'] == a / 16000.0 and seg['end'] == b / 16000.0
        assert seg['words'] == [{'word': w, 'start': a / 16000.0 + s, 'end': a / 16000.0 + e} for w, s, e in words]
        texts.append(text)
    assert got['text'] == ' '.join(t for t in texts if t.strip())
    assert any(t.strip() for t in texts), 'the random model transcribes these bursts as nothing: the comparison shows nothing'
    plain = model.transcribe_long(x, batch_size=1)[0]
    assert plain['text'] == got['text'] and all('words' not in s for s in plain['segments'])
    # batched pieces keep their order and times
    batched = model.transcribe_long([x, x[:40000]], batch_size=8)
    assert [(s['start'], s['end']) for s in batched[0]['segments']] == [(s['start'], s['end']) for s in got['segments']]
    assert len(batched[1]['segments']) == 1
    # silence, and an empty recording
    quiet = model.transcribe_long([np.zeros(32000, dtype=np.float32), np.zeros(0, dtype=np.float32)])
    assert quiet == [{'text': '', 'segments': []}] * 2
    # 48 kHz: the segments (and text) of its resampled waveform
    x48 = _speechlike(2, ((0.4, 1.4), (2.2, 3.0)), 3.6, rate=48000)
    up, n_up = resample_batch([x48], [48000], 16000)
    want = model.transcribe_long([up[0, :int(n_up[0])]], batch_size=1)[0]
    got48 = model.transcribe_long([(x48, 48000)], batch_size=1)[0]
    assert got48 == want and len(want['segments']) == 2


def test_transcribe_long_under_asg(monkeypatch):
    """a model with criterion asg: text through its own Viterbi decoder; word times keep decode_batch's refusal"""
    from asg_replay_worker import build_model
    monkeypatch.setattr('wav2letter_pytorch_amd.data.data_loader.SpectrogramExtractor.dithering', 0.0)
    asg = build_model(seed=6).cuda().eval()
    x = _speechlike(4, ((0.4, 1.2), (2.0, 2.9)), 3.5)
    got = asg.transcribe_long([x], batch_size=1)[0]
    assert len(got['segments']) == 2
    for seg in got['segments']:
        a, b = int(round(seg['start'] * 16000)), int(round(seg['end'] * 16000))
        assert seg['text'] == asg.transcribe([x[a:b]], batch_size=1)[0]
    with pytest.raises(NotImplementedError):
        asg.transcribe_long([x], word_times=True)


def test_device_rows_features_bit_equal_extract_batch(model, monkeypatch):
    monkeypatch.setattr('wav2letter_pytorch_amd.data.data_loader.SpectrogramExtractor.dithering', 0.0)
    model.transcribe_long([np.zeros(1600, dtype=np.float32)])               # (creates the extractor)
    ext = model._transcribe_extractor
    g = np.random.default_rng(9)
    sigs = [(0.2 * g.standard_normal(n)).astype(np.float32) for n in (9000, 4001, 12345)]
    want, want_lens = ext.extract_batch(sigs, noise=False)
    rows = torch.zeros(3, 12345, device='cuda')
    for i, s in enumerate(sigs):
        rows[i, :len(s)] = torch.from_numpy(s).cuda()
    got, got_lens = ext.extract_rows(rows, [len(s) for s in sigs], noise=False)
    assert got_lens.tolist() == want_lens.tolist()
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    with pytest.raises(ValueError):
        ext.extract_rows(rows, [9000, 200, 12345])       # at or under the reflect padding
    with pytest.raises(ValueError):
        ext.extract_rows(rows.cpu(), [9000, 4001, 12345])


def test_transcribe_long_needs_less_memory_than_the_whole_file(model, monkeypatch):
    monkeypatch.setattr('wav2letter_pytorch_amd.data.data_loader.SpectrogramExtractor.dithering', 0.0)
    rec = np.concatenate([VC.synthetic_recording(s, -60.0) for s in range(8)])          # 240 s
    # the peak is taken above what is allocated when the call starts: whatever ran earlier in the process (other tests' models,
    # the engine's caches) is in max_memory_allocated too and is no cost of either call.  Both calls have run once before, so
    # that what they leave behind (the extractor, tuned shapes, the inference state) is part of that baseline for both.
    runs = (lambda: model.transcribe_long([rec], max_seconds=15.0), lambda: model.transcribe([rec], batch_size=1))
    for run in runs:
        run()
    peaks = []
    for run in runs:
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = run()
        torch.cuda.synchronize()
        peaks.append(torch.cuda.max_memory_allocated() - base)
    print(f'peak memory: transcribe_long {peaks[0] / 2 ** 20:.1f} MiB, transcribe of the whole file {peaks[1] / 2 ** 20:.1f} MiB')
    assert peaks[0] < peaks[1]
    assert isinstance(out[0], str)


def test_transcribe_command_line(model, tmp_path, monkeypatch):
    from wav2letter_pytorch_amd import transcribe as TR
    from wav2letter_pytorch_amd.data.data_loader import read_audio
    monkeypatch.setattr('wav2letter_pytorch_amd.data.data_loader.SpectrogramExtractor.dithering', 0.0)
    paths = []
    for i, bursts in enumerate((((0.5, 1.5), (2.5, 3.3)), ((0.3, 1.0),))):
        sig = _speechlike(20 + i, bursts, 4.0 - i)
        p = str(tmp_path / f'rec{i}.wav')
        with wave.open(p, 'wb') as f:
            f.setnchannels(1); f.setsampwidth(2); f.setframerate(16000)
            f.writeframes((np.clip(sig, -1, 1) * 32767).astype('<i2').tobytes())
        paths.append(p)
    ckpt = str(tmp_path / 'model.ckpt')
    torch.save({'state_dict': model.state_dict()}, ckpt)
    out = str(tmp_path / 'out.jsonl')
    records = TR.main([f'model_path={ckpt}', 'audio=' + ','.join(paths), 'model.mid_layers=1', 'segment.max_seconds=15', 'batch_size=1',
                       'word_times=true', f'output={out}'])
    lines = [json.loads(l) for l in open(out)]
    assert [l['path'] for l in lines] == paths and lines == json.loads(json.dumps(records))
    want = model.transcribe_long([read_audio(p)[0] for p in paths], max_seconds=15.0, batch_size=1, word_times=True)
    for line, w in zip(lines, want):
        assert line['text'] == w['text'] and line['segments'] == json.loads(json.dumps(w['segments']))
    assert [len(l['segments']) for l in lines] == [2, 1]
    beam = TR.main([f'model_path={ckpt}', f'audio={paths[1]}', 'model.mid_layers=1', 'decoder=beam', 'beam.k=3'])
    assert len(beam) == 1 and len(beam[0]['segments']) == 1 and 'words' not in beam[0]['segments'][0]
