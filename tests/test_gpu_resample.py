"""The sample-rate converter on a real MI355X: w2l_resample through the C ABI against the float64 reference
(tests/resample_refs.py) under the derived fp32 dot-product bound, its argument checks, and what is built on it --
SpectrogramExtractor.extract_batch(rates=, speeds=), ConvCTCASR.transcribe on files of other rates, the loader with
resample=True and speed perturbation, the train command line."""
import json
import os
import random
import sys
import wave

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resample_refs as RR  # noqa: E402

pytestmark = pytest.mark.gpu

CONF = dict(window='hamming', window_stride=0.01, window_size=0.02, sample_rate=16000)
TILE = 512                       # W2L_RESAMPLE_TILE

# the rows of one launch: (P, Q, n_in).  Row 4 is shorter than the filter's reach, row 6 is copied.
ROWS = [(3, 1, 4099), (1, 2, 1537), (441, 160, 10007), (9, 10, 7), (11, 10, 3001), (1, 1, 2500)]


def _launch(x, rows, cache, out_stride=None):
    """x fp32 [N, L] on the device, rows int32 [N, 5] -> out [N, out_stride] through the C ABI"""
    from wav2letter_pytorch_amd._lib import check, lib, ptr, stream_ptr
    taps, desc_dev = cache.device_tables(x.device)
    rows = np.ascontiguousarray(rows, dtype=np.int32)
    rows_dev = torch.from_numpy(rows).to(x.device)
    out_stride = int(rows[:, 1].max()) if out_stride is None else out_stride
    out = torch.full((x.shape[0], out_stride), 7.0, dtype=torch.float32, device=x.device)
    desc = np.ascontiguousarray(cache.desc)
    check(lib.w2l_resample(ptr(x), x.shape[1], ptr(out), out_stride, x.shape[0], rows.ctypes.data, ptr(rows_dev), desc.ctypes.data,
                           ptr(desc_dev), len(desc), ptr(taps), taps.numel(), stream_ptr()), 'w2l_resample')
    torch.cuda.synchronize()
    return out


def test_kernel_against_float64_reference_mixed_ratios_in_one_launch():
    from wav2letter_pytorch_amd.data.resample import BankCache, filter_bank
    g = np.random.default_rng(11)
    cache = BankCache()
    sig = [(0.5 * g.standard_normal(n)).astype(np.float32) for _, _, n in ROWS]
    rows = np.array([(n, RR.n_out_ref(n, P, Q), P, Q, -1 if P == Q else cache.bank(P, Q)) for P, Q, n in ROWS], dtype=np.int32)
    n_outs = rows[:, 1]
    assert n_outs.max() > TILE and all(int(v) % TILE for v in n_outs)       # more than one tile; no row ends on a tile edge
    assert rows[3, 0] < filter_bank(9, 10)[1]                               # row 4 is shorter than H
    L = max(n for _, _, n in ROWS) + 1                                      # 10008: 16-byte aligned rows, the vector loads' path
    assert L % 4 == 0                                                       # (the long row below has an odd stride: scalar loads)
    x = np.full((len(ROWS), L), 3.0, dtype=np.float32)                      # beyond n_in: NOT zero -- the kernel must not read it
    for i, s in enumerate(sig):
        x[i, :s.shape[0]] = s
    stride = int(n_outs.max()) + 5                                          # a row stride that is no multiple of 4 or of the tile
    out = _launch(torch.from_numpy(x).cuda(), rows, cache, stride).cpu().numpy()
    for i, (P, Q, n) in enumerate(ROWS):
        no = int(n_outs[i])
        assert not out[i, no:].any(), f'row {i}: columns past n_out are not zero'
        if P == Q:
            np.testing.assert_array_equal(out[i, :no].view(np.uint32), sig[i].view(np.uint32))
            continue
        h, H = filter_bank(P, Q)
        ref, A = RR.resample_ref(sig[i], P, Q, h)
        assert ref.shape[0] == no
        err = np.abs(out[i, :no].astype(np.float64) - ref)
        bound = RR.resample_bound(A, h.shape[1], ref)
        worst = int(np.argmax(err - bound))
        print(f'row {i} ({P}/{Q}, n_in {n}, K {h.shape[1]}): max err {err.max():.3e}, max err/bound {np.max(err / np.maximum(bound, 1e-300)):.3f}')
        assert (err <= bound).all(), (i, worst, err[worst], bound[worst])


def test_long_row_index_arithmetic_past_2_to_the_32():
    """4851/1600 (44.1 kHz at speed 1.1) over 3 000 017 samples: m P passes 2^31 and 2^32; the reference is evaluated on the
    first and last 4096 outputs and 4096 around each crossing"""
    from wav2letter_pytorch_amd.data.resample import BankCache, filter_bank
    P, Q, n_in = 4851, 1600, 3000017
    g = np.random.default_rng(12)
    sig = (0.5 * g.standard_normal(n_in)).astype(np.float32)
    cache = BankCache()
    n_out = RR.n_out_ref(n_in, P, Q)
    rows = np.array([(n_in, n_out, P, Q, cache.bank(P, Q))], dtype=np.int32)
    out = _launch(torch.from_numpy(sig).cuda()[None], rows, cache)[0].cpu().numpy()
    h, _ = filter_bank(P, Q)
    windows = [(0, 4096), (n_out - 4096, n_out)]
    for power in (31, 32):
        m_cross = (1 << power) // P
        assert 2048 < m_cross < n_out - 2048
        windows.append((m_cross - 2048, m_cross + 2048))
    for lo, hi in windows:
        ref, A = RR.resample_ref(sig, P, Q, h, lo, hi)
        err = np.abs(out[lo:hi].astype(np.float64) - ref)
        bound = RR.resample_bound(A, h.shape[1], ref)
        print(f'outputs [{lo}, {hi}): max err {err.max():.3e}, max err/bound {np.max(err / np.maximum(bound, 1e-300)):.3f}')
        assert (err <= bound).all(), (lo, hi)


def test_argument_checks_return_the_error_code_and_launch_nothing():
    from wav2letter_pytorch_amd._lib import lib, ptr, stream_ptr
    from wav2letter_pytorch_amd.data.resample import BankCache
    cache = BankCache()
    b = cache.bank(3, 1)
    taps, desc_dev = cache.device_tables(torch.device('cuda', torch.cuda.current_device()))
    x = torch.ones(1, 3000, device='cuda')
    out = torch.full((1, 1000), 7.0, device='cuda')
    good = np.array([[3000, 1000, 3, 1, b]], dtype=np.int32)

    def call(rows=good, desc=cache.desc, x_=x, out_=out, rows_dev=True, taps_=taps, out_stride=1000):
        rows = np.ascontiguousarray(rows, dtype=np.int32)
        desc = np.ascontiguousarray(desc, dtype=np.int32)
        rd = torch.from_numpy(rows).cuda() if rows_dev else None
        dd = torch.from_numpy(desc).cuda()
        rc = lib.w2l_resample(ptr(x_), 3000, ptr(out_), out_stride, 1, rows.ctypes.data, ptr(rd), desc.ctypes.data, ptr(dd), len(desc),
                              ptr(taps_), 0 if taps_ is None else taps_.numel(), stream_ptr())
        torch.cuda.synchronize()
        return rc

    def row(**kw):
        r = dict(n_in=3000, n_out=1000, P=3, Q=1, bank=b)
        r.update(kw)
        return np.array([[r['n_in'], r['n_out'], r['P'], r['Q'], r['bank']]], dtype=np.int32)

    bad_desc = cache.desc.copy()
    bad_desc[0, 1:3] = (2 * 300 + 2, 300)                # K = 602 > W2L_RESAMPLE_MAX_K
    cases = {
        'null input': dict(x_=None), 'null output': dict(out_=None), 'null device rows': dict(rows_dev=False),
        'null taps': dict(taps_=None),
        'P = 0': dict(rows=row(P=0)), 'Q < 0': dict(rows=row(Q=-1)),
        'n_out too small': dict(rows=row(n_out=999)), 'n_out too large': dict(rows=row(n_out=1001)),
        'n_in past the stride': dict(rows=row(n_in=3003, n_out=1001)),
        'n_out past the stride': dict(out_stride=999),
        'bank out of range': dict(rows=row(bank=1)), 'negative bank': dict(rows=row(bank=-1)),
        'bank of another Q': dict(rows=row(P=3, Q=2, n_in=1500, n_out=1000)),
        'K above the maximum': dict(desc=bad_desc),
    }
    for name, kw in cases.items():
        assert call(**kw) != 0, name
        assert lib.w2l_last_error(), name
        assert bool((out == 7.0).all()), f'{name}: something was launched'
    assert call() == 0 and bool((out != 7.0).all())


@pytest.fixture(scope='module')
def ext():
    from wav2letter_pytorch_amd.data.data_loader import SpectrogramExtractor
    e = SpectrogramExtractor(CONF, 64)
    e.dithering = 0.0
    return e


def test_extract_batch_composes_resampling_and_features_bit_exactly(ext):
    from wav2letter_pytorch_amd.data.resample import resample_batch
    g = np.random.default_rng(13)
    rates = [48000, 8000, 44100, 16000, 16000]
    speeds = [1.0, 1.1, 0.9, 1.0, 1.1]
    sig = [(0.2 * g.standard_normal(n)).astype(np.float32) for n in (20011, 3001, 17003, 5000, 6007)]
    audio, n_out = resample_batch(sig, rates, 16000, speeds)
    want_n = [RR.n_out_ref(len(s), *_pq(r, sp)) for s, r, sp in zip(sig, rates, speeds)]
    assert n_out.tolist() == want_n and audio.shape == (5, max(want_n))
    got, got_len = ext.extract_batch(sig, rates=rates, speeds=speeds)
    rows = [audio[i, :int(n_out[i])].cpu().numpy() for i in range(5)]
    assert np.array_equal(rows[3], sig[3])                                   # model rate, speed 1: copied
    want, want_len = ext.extract_batch(rows)
    assert torch.equal(got, want) and torch.equal(got_len, want_len)
    assert got_len.dtype == torch.int32 and got_len.tolist() == [1 + n // ext.hop_length for n in want_n]
    # rows at the model's rate and speed 1: the plain extract_batch, whichever argument is given
    plain, plain_len = ext.extract_batch(sig[3:])
    for kw in (dict(rates=[16000, 16000]), dict(speeds=[1.0, 1]), dict(rates=[16000, 16000], speeds=[1, 1.0])):
        again, again_len = ext.extract_batch(sig[3:], **kw)
        assert torch.equal(again, plain) and torch.equal(again_len, plain_len)
    # the STFT's length rule applies to the resampled length: 600 samples at 48 kHz are 200 at 16 kHz
    with pytest.raises(ValueError):
        ext.extract_batch([sig[0][:600]], rates=[48000])
    ext.extract_batch([sig[0][:600]], rates=[16000])


def _pq(rate, speed):
    from wav2letter_pytorch_amd.data.resample import resample_ratio
    r = resample_ratio(rate, 16000, speed)
    return r.numerator, r.denominator


def _write_wav(path, samples, sr, channels=1):
    """samples float [n] or [n, channels] -> 16-bit PCM"""
    with wave.open(str(path), 'wb') as w:
        w.setnchannels(channels)
        w.setsampwidth(2)
        w.setframerate(sr)
        w.writeframes((np.clip(samples, -1, 1) * 32767).astype('<i2').tobytes())


def _pcm(samples):
    """what a 16-bit file written by _write_wav reads back as"""
    return (np.clip(samples, -1, 1) * 32767).astype('<i2').astype(np.float32) / 32768.0


def test_transcribe_reads_any_rate_and_channel_count(tmp_path, monkeypatch):
    from wav2letter_pytorch_amd import Wav2Letter
    from wav2letter_pytorch_amd.data.data_loader import load_audio, read_audio
    from wav2letter_pytorch_amd.data.resample import resample_batch
    from wav2letter_pytorch_amd.defaults import wav2letter_model
    monkeypatch.setattr('wav2letter_pytorch_amd.data.data_loader.SpectrogramExtractor.dithering', 0.0)
    torch.manual_seed(7)
    model = Wav2Letter(wav2letter_model(mid_layers=1, dropout=False)).cuda().eval()
    g = np.random.default_rng(14)
    a8 = 0.3 * g.standard_normal(6000)                                      # 0.75 s at 8 kHz
    st = 0.3 * g.standard_normal((11000, 2))                                # stereo at 16 kHz
    m16 = 0.3 * g.standard_normal(9000)
    p8, pst, p16 = (str(tmp_path / n) for n in ('a8.wav', 'st.wav', 'm16.wav'))
    _write_wav(p8, a8, 8000)
    _write_wav(pst, st, 16000, channels=2)
    _write_wav(p16, m16, 16000)
    w8, r8 = read_audio(p8)
    assert r8 == 8000 and np.array_equal(w8, _pcm(a8))
    wst, rst = read_audio(pst)
    mean = _pcm(st).mean(axis=1, dtype=np.float32)
    assert rst == 16000 and wst.ndim == 1 and np.array_equal(wst, mean)
    assert load_audio(pst).shape == (2, 11000)                              # load_audio keeps the reference's return value
    # one item per call: Wav2Letter's reflection padding makes an utterance's text depend on its batch
    from_path = model.transcribe(p8)
    from_wave = model.transcribe([(w8, 8000)])
    up, n_up = resample_batch([w8], [8000], 16000)
    assert int(n_up[0]) == 12000
    from_resampled = model.transcribe([up[0].cpu().numpy()])
    assert from_path == from_wave == from_resampled and len(from_path) == 1
    assert model.transcribe(pst) == model.transcribe([mean])
    assert model.transcribe(p16) == model.transcribe([load_audio(p16)])
    # a mixed chunk: the same features as extract_batch with the files' rates
    ext = model._transcribe_extractor
    x, lens = ext.extract_batch([w8, wst, load_audio(p16)], rates=[8000, 16000, 16000])
    assert lens.tolist() == [1 + 12000 // 160, 1 + 11000 // 160, 1 + 9000 // 160]
    with torch.no_grad():
        out, out_lens = model.infer(x, lens)
    from wav2letter_pytorch_amd.evaluate import decode_batch
    texts = model.transcribe([p8, pst, p16], batch_size=3)
    assert texts == decode_batch(model, model.ctc_decoder, out, out_lens, False)[0]
    print('transcripts:', from_path, texts)


def _manifest(tmp_path, name='m.json', first_rate=8000):
    g = np.random.default_rng(15)
    rows = []
    for i, (sr, secs) in enumerate(((first_rate, 0.8), (16000, 0.7), (8000, 0.9), (16000, 0.6))):
        p = str(tmp_path / f'{name}_{i}.wav')
        _write_wav(p, 0.2 * g.standard_normal(int(sr * secs)), sr)
        rows.append({'audio_filepath': p, 'text': ('speech on mi', 'three fifty', 'five x', 'runs fast')[i], 'rate': sr,
                     'n': int(sr * secs)})
    path = str(tmp_path / name)
    with open(path, 'w') as f:
        for r in rows:
            f.write(json.dumps({k: r[k] for k in ('audio_filepath', 'text')}) + '\n')
    return path, rows


def test_loader_resamples_per_row_and_applies_the_drawn_speeds(tmp_path):
    from wav2letter_pytorch_amd.data import label_sets
    from wav2letter_pytorch_amd.data.data_loader import BatchAudioDataLoader, SpectrogramDataset
    from wav2letter_pytorch_amd.data.resample import SpeedPerturb
    labels = label_sets.labels_map['english_lowercase']
    man, rows = _manifest(tmp_path)
    # without resample=True the first row's rate is still asserted
    with pytest.raises(AssertionError, match='Expected sample rate 16000 but found 8000'):
        SpectrogramDataset(man, CONF, labels, mel_spec=64)
    factors = (0.9, 1.0, 1.1)
    ds = SpectrogramDataset(man, CONF, labels, mel_spec=64, resample=True, speed_perturb=SpeedPerturb(factors, rng=random.Random(21)))
    ds.extractor.dithering = 0.0
    drawn = SpeedPerturb(factors, rng=random.Random(21)).draw(4)
    assert len(set(drawn)) > 1
    batches = list(BatchAudioDataLoader(ds, batch_size=2))
    got = [int(v) for b in batches for v in b[1]]
    want = [1 + RR.n_out_ref(r['n'], *_pq(r['rate'], s)) // 160 for r, s in zip(rows, drawn)]
    assert got == want
    assert batches[0][0].shape == (2, 64, max(want[:2])) and batches[1][0].shape == (2, 64, max(want[2:]))
    assert [ds.rate(i) for i in range(4)] == [r['rate'] for r in rows]
    # dataset[i] is never perturbed: the features of the row at the model's rate
    spect = ds[0][0]
    assert spect.shape == (64, 1 + 2 * rows[0]['n'] // 160)
    # no speed_perturb: lengths follow the rates alone
    ds2 = SpectrogramDataset(man, CONF, labels, mel_spec=64, resample=True)
    got2 = [int(v) for b in BatchAudioDataLoader(ds2, batch_size=4) for v in b[1]]
    assert got2 == [1 + RR.n_out_ref(r['n'], *_pq(r['rate'], 1)) // 160 for r in rows]


def test_train_cli_resample_and_speed_perturb(tmp_path):
    """`python -m wav2letter_pytorch_amd.train ... data.resample=true data.speed_perturb=0.9,1.0,1.1` on a manifest of two
    sample rates: two steps run; the validation loader gets no perturbation"""
    from wav2letter_pytorch_amd.train import main
    man, _ = _manifest(tmp_path)
    out = tmp_path / 'run'
    trainer, model = main([f'data.train_manifest={man}', f'data.val_manifest={man}', 'data.batch_size=2', 'model.mid_layers=1',
                           'data.resample=true', 'data.speed_perturb=0.9,1.0,1.1', 'trainer.max_steps=2',
                           f'trainer.default_root_dir={out}'])
    assert trainer.global_step == 2 and np.isfinite(trainer.logged[-1][1]['train_loss'])
    from wav2letter_pytorch_amd.train import build_config, get_data_loaders
    from wav2letter_pytorch_amd.data import label_sets
    cfg = build_config([f'data.train_manifest={man}', f'data.val_manifest={man}', 'data.resample=true', 'data.speed_perturb=0.9,1.0,1.1'])
    tr, va = get_data_loaders(list(label_sets.labels_map['english_lowercase']), cfg.data)
    assert tr._spect_ds.resample and va._spect_ds.resample
    assert tr._spect_ds.speed_perturb.factors == (0.9, 1.0, 1.1) and va._spect_ds.speed_perturb is None
