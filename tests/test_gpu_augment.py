"""The waveform augmentations on a real MI355X: w2l_reverb and w2l_mix_noise through the C ABI against the float64 references
(tests/augment_refs.py) under derived fp32 bounds, their edge cases, and what is built on them -- WaveformAugment in
SpectrogramDataset / BatchAudioDataLoader, the train command line.

Bounds.  Reverberation: K fp32 products accumulated by fmaf in a few separately rounded chains that are then added,
|err[m]| <= 1.01 (K + 64) 2^-24 sum_j |h[j]| |x~[m + d - j]| + 1e-30.  Mixing: g is rounded once to fp32 and the fmaf rounds
once, |err| <= 4 2^-24 (|x| + |g z|) + 1e-30.  Features behind the augmentation: 2e-4 absolute on the normalised log-mel
values, the gate test_gpu_features.py puts on the front end's own fp32 rounding against its float64 oracle -- the waveforms
fed to it here differ from the device's by parts in 10^6 of their level (the bounds above, K < 1000), which moves
unit-variance features by an order less than that gate."""
import json
import os
import random
import re
import sys
import wave

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import augment_refs as AR  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONF = dict(window='hamming', window_stride=0.01, window_size=0.02, sample_rate=16000)
_HDR = dict(re.findall(r'#define (W2L_(?:REVERB|MIX)_\w+) (\d+)', open(os.path.join(ROOT, 'include', 'w2l_hip.h')).read()))
TILE, CHUNK, MAX_TAPS, MIX_TILE = (int(_HDR[k]) for k in ('W2L_REVERB_TILE', 'W2L_REVERB_CHUNK', 'W2L_REVERB_MAX_TAPS', 'W2L_MIX_TILE'))
FEATURE_TOL = 2e-4


# ---------------------------------------------------------------------------------------------------------------- w2l_reverb
N_INS = [1, TILE - 1, TILE, TILE + 1, 3 * TILE + 7]
L_IN = N_INS[-1] + 2                                     # row strides that are no multiple of 4 (or of each other)
L_OUT = N_INS[-1] + 6
assert L_IN % 4 and L_OUT % 4


def _reverb(x, rows, bank, out_stride):
    """x fp32 [N, L] on the device, rows int32 [N, 2] -> out [N, out_stride] through the C ABI (output prefilled with 7)"""
    from wav2letter_pytorch_amd._lib import check, lib, ptr, stream_ptr
    taps, desc_dev = bank.device_tables(x.device)
    rows = np.ascontiguousarray(rows, dtype=np.int32)
    rows_dev = torch.from_numpy(rows).to(x.device)
    out = torch.full((x.shape[0], out_stride), 7.0, dtype=torch.float32, device=x.device)
    desc = np.ascontiguousarray(bank.desc)
    check(lib.w2l_reverb(ptr(x), x.shape[1], ptr(out), out_stride, x.shape[0], rows.ctypes.data, ptr(rows_dev),
                         desc.ctypes.data if len(desc) else None, ptr(desc_dev), len(desc), ptr(taps),
                         0 if taps is None else taps.numel(), stream_ptr()), 'w2l_reverb')
    torch.cuda.synchronize()
    return out


@pytest.fixture(scope='module')
def signals():
    """one signal per length, shared by every case; beyond n_in the rows hold 3.0, which the kernel must not read"""
    g = np.random.default_rng(31)
    return {n: (0.5 * g.standard_normal(n)).astype(np.float32) for n in N_INS}


@pytest.mark.parametrize('K', [1, 2, 31, 32, 33, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 5])
def test_reverb_against_float64_reference(K, signals):
    """every (d, n_in) pair of d in {0, K - 1, mid} x n_in in {1, tile - 1, tile, tile + 1, 3 tile + 7} (K > n_in among them),
    in launches of 3 rows with three different lengths and three different responses"""
    from wav2letter_pytorch_amd.data.augment_wave import RirBank
    g = np.random.default_rng(1000 + K)
    ds = [0, K - 1, K // 2]
    hs = [(g.standard_normal(K) * np.exp(-np.arange(K) / 300.0)).astype(np.float32) for _ in ds]
    bank = RirBank(list(zip(hs, ds)))
    refs = {}
    worst = 0.0
    for shift in range(5):
        ns = [N_INS[(shift + 2 * r) % 5] for r in range(3)]
        assert len(set(ns)) == 3
        x = np.full((3, L_IN), 3.0, dtype=np.float32)
        for r, n in enumerate(ns):
            x[r, :n] = signals[n]
        rows = np.array([(n, r) for r, n in enumerate(ns)], dtype=np.int32)
        xd = torch.from_numpy(x).cuda()
        out = _reverb(xd, rows, bank, L_OUT)
        if shift == 0:
            assert torch.equal(out, _reverb(xd, rows, bank, L_OUT)), 'two calls differ'
        out = out.cpu().numpy()
        for r, n in enumerate(ns):
            assert not out[r, n:].any(), f'K {K}, row {r}: columns past n_in = {n} are not zero'
            if (r, n) not in refs:
                refs[r, n] = AR.reverb_ref(signals[n], hs[r], ds[r])
            ref, A = refs[r, n]
            err = np.abs(out[r, :n].astype(np.float64) - ref)
            bound = AR.reverb_bound(A, K)
            worst = max(worst, float(np.max(err / bound)))
            at = int(np.argmax(err - bound))
            assert (err <= bound).all(), (K, ds[r], n, at, err[at], bound[at])
    print(f'K {K}: max err / bound {worst:.3f} over {len(refs)} (d, n_in) pairs')


def test_reverb_row_without_a_response_is_a_bit_copy(signals):
    from wav2letter_pytorch_amd.data.augment_wave import RirBank, reverb_device
    g = np.random.default_rng(32)
    h = g.standard_normal(40).astype(np.float32)
    bank = RirBank([(h, 5)])
    ns = [TILE + 1, 3 * TILE + 7, TILE - 1]
    x = np.full((3, L_IN), 3.0, dtype=np.float32)
    for r, n in enumerate(ns):
        x[r, :n] = signals[n]
    rows = np.array([(ns[0], 0), (ns[1], -1), (ns[2], 0)], dtype=np.int32)
    out = _reverb(torch.from_numpy(x).cuda(), rows, bank, L_OUT).cpu().numpy()
    np.testing.assert_array_equal(out[1, :ns[1]].view(np.uint32), signals[ns[1]].view(np.uint32))
    assert not out[1, ns[1]:].any() and not out[0, ns[0]:].any() and not out[2, ns[2]:].any()
    for r in (0, 2):
        ref, A = AR.reverb_ref(signals[ns[r]], h, 5)
        assert (np.abs(out[r, :ns[r]] - ref) <= AR.reverb_bound(A, 40)).all()
    # the module's entry point: same rows, input zero-padded as the loader stages it, output of the input's shape
    xz = x.copy()
    for r, n in enumerate(ns):
        xz[r, n:] = 0.0
    got = reverb_device(torch.from_numpy(xz).cuda(), rows, bank)
    assert got.shape == (3, L_IN) and np.array_equal(got.cpu().numpy(), out[:, :L_IN])
    # a batch with no response at all needs no bank
    none = reverb_device(torch.from_numpy(xz).cuda(), np.array([(n, -1) for n in ns], dtype=np.int32), RirBank())
    assert np.array_equal(none.cpu().numpy(), xz)


def test_reverb_refuses_more_taps_than_the_limit():
    from wav2letter_pytorch_amd._lib import W2LError, check, lib, ptr, stream_ptr
    K = MAX_TAPS + 1
    assert K == 16385
    x = torch.ones(1, 64, device='cuda')
    out = torch.full((1, 64), 7.0, device='cuda')
    taps = torch.ones(K, device='cuda')
    rows = np.array([[64, 0]], dtype=np.int32)

    def call(desc):
        desc = np.array([desc], dtype=np.int32)
        check(lib.w2l_reverb(ptr(x), 64, ptr(out), 64, 1, rows.ctypes.data, ptr(torch.from_numpy(rows).cuda()), desc.ctypes.data,
                             ptr(torch.from_numpy(desc).cuda()), 1, ptr(taps), K, stream_ptr()), 'w2l_reverb')
        torch.cuda.synchronize()

    with pytest.raises(W2LError, match=str(MAX_TAPS)):
        call((0, K, 0))
    for bad in ((0, 0, 0), (0, 8, 8), (0, 8, -1), (K - 4, 8, 0), (-1, 8, 0)):
        with pytest.raises(W2LError):
            call(bad)
    assert bool((out == 7.0).all()), 'something was launched'
    call((0, MAX_TAPS, 100))                             # the limit itself runs
    assert bool((out != 7.0).all())


# ---------------------------------------------------------------------------------------------------------------- w2l_mix_noise
# (n_in, n_z, o, snr_db, kind): lengths from one sample to several tiles in one launch
MIX_ROWS = [
    (5000, 1700, 333, -5.0, 'mix'),                      # the clip wraps more than once
    (3000, 4000, 1000, 0.0, 'mix'),                      # o + n_in lands exactly on n_z
    (3000, 4000, 1001, 20.0, 'mix'),                     # ... and one past it
    (1, 10, 3, 0.0, 'mix'),
    (2500, 900, 7, 10.0, 'silent utterance'),
    (2500, 900, 7, 10.0, 'silent clip'),
    (2500, 0, 0, 10.0, 'no noise'),
    (3 * MIX_TILE + 7, 3 * MIX_TILE + 7, 0, 20.0, 'mix'),
    (MIX_TILE, 2 * MIX_TILE, MIX_TILE, -5.0, 'mix'),
]


def test_mix_noise_against_float64_reference():
    from wav2letter_pytorch_amd.data.augment_wave import mix_noise_device
    g = np.random.default_rng(33)
    N = len(MIX_ROWS)
    L = max(r[0] for r in MIX_ROWS) + 2
    Z = max(r[1] for r in MIX_ROWS) + 1
    assert L % 4 and max(r[0] for r in MIX_ROWS) > 3 * MIX_TILE and min(r[0] for r in MIX_ROWS) == 1
    x = np.zeros((N, L), dtype=np.float32)               # the loader's layout: zero past each row's end
    z = np.full((N, Z), 3.0, dtype=np.float32)           # beyond n_z: not zero -- never read
    for i, (n, nz, o, snr, kind) in enumerate(MIX_ROWS):
        if kind != 'silent utterance':
            x[i, :n] = 0.3 * g.standard_normal(n)
        z[i, :nz] = 0.0 if kind == 'silent clip' else 2.0 * g.standard_normal(nz)
    lens = np.array([r[0] for r in MIX_ROWS], dtype=np.int32)
    rows = np.array([(r[1], r[2]) for r in MIX_ROWS], dtype=np.int32)
    snr = np.array([r[3] for r in MIX_ROWS], dtype=np.float32)
    xd, zd = torch.from_numpy(x).cuda(), torch.from_numpy(z).cuda()
    out_d = mix_noise_device(xd, lens, zd, rows, snr)
    assert torch.equal(out_d, mix_noise_device(xd, lens, zd, rows, snr)), 'two calls differ'
    out = out_d.cpu().numpy()
    assert out.shape == x.shape
    for i, (n, nz, o, s, kind) in enumerate(MIX_ROWS):
        assert not out[i, n:].any(), f'row {i}: columns past n_in are not zero'
        if kind != 'mix':
            np.testing.assert_array_equal(out[i, :n].view(np.uint32), x[i, :n].view(np.uint32), err_msg=kind)
            continue
        ref, gain, zw = AR.mix_ref(x[i, :n], z[i, :nz], o, float(snr[i]))
        assert gain > 0
        err = np.abs(out[i, :n].astype(np.float64) - ref)
        bound = 4 * 2.0 ** -24 * (np.abs(x[i, :n].astype(np.float64)) + np.abs(gain * zw)) + 1e-30
        got_snr = AR.snr_db_of(x[i, :n], out[i, :n])
        print(f'row {i} (n_in {n}, n_z {nz}, o {o}): max err / bound {np.max(err / bound):.3f}, SNR {got_snr:.7f} dB for {s}')
        assert (err <= bound).all(), (i, int(np.argmax(err - bound)))
        assert abs(got_snr - s) <= 1e-4, (i, got_snr, s)
    assert {-5.0, 0.0, 20.0} <= {r[3] for r in MIX_ROWS if r[4] == 'mix' and r[0] > 1}


def test_mix_noise_argument_checks():
    from wav2letter_pytorch_amd._lib import W2LError
    from wav2letter_pytorch_amd.data.augment_wave import mix_noise_device
    x = torch.ones(2, 100, device='cuda')
    z = torch.ones(2, 50, device='cuda')
    ok = mix_noise_device(x, [100, 60], z, [(50, 49), (0, 0)], [3.0, 3.0])
    assert bool((ok[1, :60] == 1).all()) and not bool(ok[1, 60:].any())
    for lens, rows in (([101, 60], [(50, 0), (0, 0)]), ([100, 60], [(51, 0), (0, 0)]), ([100, 60], [(50, 50), (0, 0)]),
                       ([100, 60], [(50, -1), (0, 0)]), ([100, -1], [(50, 0), (0, 0)])):
        with pytest.raises(W2LError):
            mix_noise_device(x, lens, z, rows, [3.0, 3.0])


# ---------------------------------------------------------------------------------------------------------------- the chain
def _write_wav(path, samples, sr):
    with wave.open(str(path), 'wb') as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(sr)
        w.writeframes((np.clip(samples, -1, 1) * 32767).astype('<i2').tobytes())


def _rir(rate, seed):
    """a decaying noise burst with its peak at sample 37, 40 ms long"""
    g = np.random.default_rng(seed)
    n = int(0.04 * rate)
    h = 0.05 * g.standard_normal(n) * np.exp(-np.arange(n) / (0.008 * rate))     # low enough that the peak survives a 3:1 low-pass
    h[:37] *= 0.05
    h[37] = 0.95
    return h


@pytest.fixture(scope='module')
def corpus(tmp_path_factory):
    d = tmp_path_factory.mktemp('augment')
    g = np.random.default_rng(34)

    def manifest(name, items, text=None):
        path = str(d / name)
        with open(path, 'w') as f:
            for i, (samples, sr) in enumerate(items):
                p = str(d / f'{name}_{i}.wav')
                _write_wav(p, samples, sr)
                row = {'audio_filepath': p}
                if text:
                    row['text'] = text[i]
                f.write(json.dumps(row) + '\n')
        return path

    utts = manifest('utts.json', [(0.2 * g.standard_normal(11000), 16000), (0.2 * g.standard_normal(9000), 16000)],
                    text=['speech on mi', 'three fifty'])
    noise = manifest('noise.json', [(0.1 * g.standard_normal(7000), 8000), (0.4 * g.standard_normal(5000), 16000)])
    rirs = manifest('rirs.json', [(_rir(16000, 1), 16000), (_rir(48000, 2), 48000)])
    return utts, noise, rirs


def _dataset(corpus, seed=5, **kw):
    from wav2letter_pytorch_amd.data import label_sets
    from wav2letter_pytorch_amd.data.augment_wave import WaveformAugment
    from wav2letter_pytorch_amd.data.data_loader import SpectrogramDataset
    utts, noise, rirs = corpus
    labels = label_sets.labels_map['english_lowercase']
    aug = None
    if seed is not None:
        args = dict(noise_manifest=noise, rir_manifest=rirs, noise_prob=0.8, rir_prob=0.8, snr_db=(5, 20), rng=random.Random(seed))
        args.update(kw)
        aug = WaveformAugment(**args)
    ds = SpectrogramDataset(utts, CONF, labels, mel_spec=64, wave_augment=aug)
    ds.extractor.dithering = 0.0
    return ds


def test_loader_with_waveform_augmentation(corpus):
    from wav2letter_pytorch_amd.data.augment_wave import WaveformAugment
    from wav2letter_pytorch_amd.data.data_loader import BatchAudioDataLoader, read_audio
    from wav2letter_pytorch_amd.data.resample import resample_batch
    plain_ds = _dataset(corpus, seed=None)
    plain = next(iter(BatchAudioDataLoader(plain_ds, batch_size=2)))
    a = next(iter(BatchAudioDataLoader(_dataset(corpus), batch_size=2)))
    b = next(iter(BatchAudioDataLoader(_dataset(corpus), batch_size=2)))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), 'the same seed gives another batch'
    assert torch.equal(a[1], plain[1]) and a[0].shape == plain[0].shape
    assert not torch.equal(a[0], plain[0])

    # the responses as prepared: peak at 37 (the 48 kHz one: a third of 37 after resampling), unit energy, 40 ms + peak
    ds = _dataset(corpus)
    aug = ds.wave_augment
    plan = WaveformAugment(*corpus[1:], noise_prob=0.8, rir_prob=0.8, snr_db=(5, 20), rng=random.Random(5)).draw(2)
    assert plan[0].rir == 1 and plan[0].clip == 0 and plan[1].rir == 0, plan     # the 48 kHz response, the 8 kHz clip, the 16 kHz response
    assert len(aug.bank) == 2 and aug.bank.response(0)[1] == 37 and 11 <= aug.bank.response(1)[1] <= 13
    for k in range(2):
        h, _ = aug.bank.response(k)
        assert abs(float(np.sum(h.astype(np.float64) ** 2)) - 1.0) <= 1e-6 and h.shape[0] <= 37 + 8000

    # the batch against extract_batch of waveforms augmented by the float64 references from the same plan
    raws = [plain_ds.raw(i)[0] for i in range(2)]
    want_wave = []
    for x, r in zip(raws, plan):
        y = x.astype(np.float64)
        if r.rir >= 0:
            y = AR.reverb_ref(y, *aug.bank.response(r.rir))[0]
        if r.clip >= 0:
            zc, sr = read_audio(aug.noise_paths[r.clip])
            if sr != 16000:
                zd, nz = resample_batch([zc], [sr], 16000)
                zc = zd[0, :int(nz[0])].cpu().numpy()
            y = AR.mix_ref(y, zc, int(r.frac * zc.shape[0]), float(np.float32(r.snr_db)))[0]
        want_wave.append(y.astype(np.float32))
    want, want_len = plain_ds.extractor.extract_batch(want_wave)
    assert torch.equal(want_len, a[1])
    diff = float((a[0] - want).abs().max())
    print(f'plan {plan}: features differ from the float64-augmented ones by at most {diff:.3e} (gate {FEATURE_TOL})')
    assert diff <= FEATURE_TOL

    # probabilities 0: the un-augmented features bit for bit -- through extract_batch with the dither injected, so that both
    # see the same draws, and through the loader
    off = _dataset(corpus, noise_prob=0.0, rir_prob=0.0)
    g = np.random.default_rng(35)
    dither = [g.standard_normal(len(x)).astype(np.float32) for x in raws]
    ext = off.extractor
    ext.dithering = 1e-5
    got, got_len = ext.extract_batch(raws, noise=dither, augment=(off.wave_augment, off.wave_augment.draw(2)))
    base, base_len = ext.extract_batch(raws, noise=dither)
    assert torch.equal(got, base) and torch.equal(got_len, base_len)
    ext.dithering = 0.0
    c = next(iter(BatchAudioDataLoader(off, batch_size=2)))
    assert torch.equal(c[0], plain[0]) and torch.equal(c[1], plain[1])


def test_train_cli_with_noise_and_reverberation(corpus):
    """`python -m wav2letter_pytorch_amd.train ... data.noise_manifest=... data.rir_manifest=...`: two steps run and log finite
    losses; the validation loader carries no augmenter"""
    from wav2letter_pytorch_amd.data import label_sets
    from wav2letter_pytorch_amd.train import build_config, get_data_loaders, main
    utts, noise, rirs = corpus
    out = os.path.join(os.path.dirname(utts), 'run')
    args = [f'data.train_manifest={utts}', f'data.val_manifest={utts}', 'data.batch_size=2', 'model.mid_layers=1',
            f'data.noise_manifest={noise}', f'data.rir_manifest={rirs}', 'data.noise_prob=1.0', 'data.rir_prob=1.0', 'data.snr_db=0,15']
    trainer, model = main(args + ['trainer.max_steps=2', 'trainer.log_every_n_steps=1', f'trainer.default_root_dir={out}'])
    losses = [logs['train_loss'] for _, logs in trainer.logged]
    assert trainer.global_step == 2 and len(losses) == 2 and all(np.isfinite(float(v)) for v in losses), losses
    cfg = build_config(args)
    tr, va = get_data_loaders(list(label_sets.labels_map['english_lowercase']), cfg.data)
    aug = tr._spect_ds.wave_augment
    assert aug is not None and aug.active and aug.snr_db == (0.0, 15.0) and aug.noise_prob == 1.0 and len(aug.bank) == 2
    assert va._spect_ds.wave_augment is None
