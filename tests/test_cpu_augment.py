"""The host side of the waveform augmentations (data/augment_wave.py), no GPU: the float64 references (tests/augment_refs.py)
pinned against numpy's and torch's own convolutions and against the SNR they promise, prepare_rir, the draws of
WaveformAugment, the config keys, and the C ABI's declarations."""
import ctypes
import os
import random
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import augment_refs as AR  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------------- references
@pytest.mark.parametrize('n,K,d', [(1, 1, 0), (50, 7, 0), (50, 7, 6), (50, 7, 3), (5, 33, 20), (300, 64, 17)])
def test_reverb_ref_is_the_shifted_full_convolution(n, K, d):
    g = np.random.default_rng(100 * n + K + d)
    x, h = g.standard_normal(n), g.standard_normal(K)
    got, A = AR.reverb_ref(x, h, d)
    want = np.convolve(x, h)[d:d + n]
    scale = np.max(np.abs(want)) + 1e-300
    assert got.shape == (n,) and np.max(np.abs(got - want)) <= 1e-12 * scale
    # torch's conv1d is a correlation: the flipped response, with d zeros of padding on the left and K - 1 - d on the right
    xt = torch.from_numpy(np.concatenate([np.zeros(K - 1 - d), x, np.zeros(d)]))[None, None]
    wt = torch.from_numpy(h[::-1].copy())[None, None]
    tc = torch.nn.functional.conv1d(xt, wt)[0, 0].numpy()
    assert tc.shape == (n,) and np.max(np.abs(got - tc)) <= 1e-12 * scale
    wantA = np.convolve(np.abs(x), np.abs(h))[d:d + n]
    assert np.max(np.abs(A - wantA)) <= 1e-12 * (np.max(wantA) + 1e-300)


@pytest.mark.parametrize('snr', [-5.0, 0.0, 12.5, 20.0])
@pytest.mark.parametrize('n,n_z,o', [(1000, 300, 17), (1000, 2500, 1500), (1000, 2500, 1501), (1, 10, 9)])
def test_mix_ref_reaches_the_requested_snr(snr, n, n_z, o):
    g = np.random.default_rng(n + n_z + o)
    x, z = 0.3 * g.standard_normal(n), 2.0 * g.standard_normal(n_z)
    out, gain, zw = AR.mix_ref(x, z, o, snr)
    assert gain > 0 and abs(AR.snr_db_of(x, out) - snr) <= 1e-9
    assert np.array_equal(zw, np.array([z[(o + m) % n_z] for m in range(n)]))


def test_mix_ref_leaves_silent_rows_alone():
    x, z = np.arange(5.0), np.ones(3)
    assert np.array_equal(AR.mix_ref(np.zeros(5), z, 1, 10)[0], np.zeros(5))
    assert np.array_equal(AR.mix_ref(x, np.zeros(3), 1, 10)[0], x)
    assert np.array_equal(AR.mix_ref(x, np.zeros(0), 0, 10)[0], x)


# ---------------------------------------------------------------------------------------------------------------- prepare_rir
def _burst(n, peak, seed, channels=1):
    g = np.random.default_rng(seed)
    h = g.standard_normal((n, channels)) * np.exp(-np.arange(n) / 200.0)[:, None] * 0.2
    h[:peak] *= 0.05
    h[peak] = 1.0 if channels == 1 else (0.9, 1.1)[:channels]
    return h[:, 0] if channels == 1 else h


def test_prepare_rir_keeps_the_peak_cuts_the_tail_and_normalises():
    from wav2letter_pytorch_amd.data.augment_wave import prepare_rir
    raw = _burst(12000, 37, 1)
    h, d = prepare_rir(raw, 16000, 16000, max_seconds=0.25)
    assert d == 37 and h.dtype == np.float32 and h.shape == (37 + 4000,)
    assert int(np.argmax(np.abs(h))) == d
    assert abs(float(np.sum(h.astype(np.float64) ** 2)) - 1.0) <= 1e-6
    want, wd = AR.prepare_rir_ref(raw, 16000, 0.25)
    assert wd == d and np.array_equal(h, want)
    # shorter than the cut: kept whole
    h2, d2 = prepare_rir(raw[:500], 16000, 16000, max_seconds=0.5)
    assert h2.shape == (500,) and d2 == 37


def test_prepare_rir_peak_at_sample_zero_and_stereo():
    from wav2letter_pytorch_amd.data.augment_wave import prepare_rir
    raw = _burst(3000, 0, 2)
    h, d = prepare_rir(raw, 16000, 16000, max_seconds=0.1)
    assert d == 0 and h.shape == (1600,) and abs(float(np.sum(h.astype(np.float64) ** 2)) - 1.0) <= 1e-6
    st = _burst(3000, 37, 3, channels=2)
    hs, ds = prepare_rir(st, 16000, 16000, max_seconds=0.1)
    hm, dm = prepare_rir(st.mean(axis=1), 16000, 16000, max_seconds=0.1)
    assert ds == dm == 37 and np.array_equal(hs, hm) and hs.shape == (37 + 1600,)
    want, _ = AR.prepare_rir_ref(st, 16000, 0.1)
    assert np.array_equal(hs, want)


def test_rir_bank_tables_and_cap():
    from wav2letter_pytorch_amd.data import augment_wave as W
    bank = W.RirBank()
    assert bank.add(np.ones(5, dtype=np.float32), 2) == 0 and bank.add(np.ones(9, dtype=np.float32), 0) == 1
    assert bank.desc.tolist() == [[0, 5, 2], [5, 9, 0]] and bank.desc.dtype == np.int32 and len(bank) == 2
    with pytest.raises(ValueError):
        bank.add(np.ones(5, dtype=np.float32), 5)        # d outside the response
    with pytest.raises(ValueError):
        bank.add(np.ones(W.MAX_TAPS + 1, dtype=np.float32), 0)
    small = W.RirBank()
    old, W.MAX_BANK_BYTES = W.MAX_BANK_BYTES, 4 * 20
    try:
        small.add(np.ones(16, dtype=np.float32), 0)
        with pytest.raises(ValueError, match='cap'):
            small.add(np.ones(5, dtype=np.float32), 0)
    finally:
        W.MAX_BANK_BYTES = old
    assert W.MAX_BANK_BYTES == 256 << 20


# ---------------------------------------------------------------------------------------------------------------- draws
class _CountingRandom(random.Random):
    def __init__(self, seed):
        super().__init__(seed)
        self.calls = 0

    def random(self):
        self.calls += 1
        return super().random()


def _augment(rng, noise=4, rirs=3, **kw):
    """a WaveformAugment with lists of names in place of manifests: draw() needs only their lengths"""
    from wav2letter_pytorch_amd.data.augment_wave import WaveformAugment
    a = WaveformAugment(rng=rng, **kw)
    a.noise_paths = ['n%d.wav' % i for i in range(noise)]
    a.rir_paths = ['r%d.wav' % i for i in range(rirs)]
    return a


def test_draws_are_reproducible_and_inside_their_ranges():
    p1 = _augment(random.Random(5), snr_db=(3, 17)).draw(200)
    p2 = _augment(random.Random(5), snr_db=(3, 17)).draw(200)
    assert p1 == p2 and p1 != _augment(random.Random(6), snr_db=(3, 17)).draw(200)
    picked = [r for r in p1 if r.clip >= 0]
    assert 50 < len(picked) < 150 and 50 < sum(r.rir >= 0 for r in p1) < 150
    assert all(3 <= r.snr_db <= 17 and 0 <= r.clip < 4 and 0.0 <= r.frac < 1.0 for r in picked)
    assert all(-1 <= r.rir < 3 for r in p1) and {r.rir for r in p1} == {-1, 0, 1, 2}
    for n_z in (1, 7, 16000):                            # the offset the loader derives lies inside the clip
        assert all(0 <= int(r.frac * n_z) < n_z for r in picked)
    assert all(r.snr_db == 0.0 and r.frac == 0.0 for r in p1 if r.clip < 0)


def test_probability_zero_selects_nothing_but_consumes_two_draws_per_utterance():
    rng = _CountingRandom(9)
    plan = _augment(rng, noise_prob=0.0, rir_prob=0.0).draw(10)
    assert all(r.rir == -1 and r.clip == -1 for r in plan) and rng.calls == 20
    # and the stream is where two random() per utterance leave it
    twin = random.Random(9)
    for _ in range(20):
        twin.random()
    assert rng.getstate() == twin.getstate()


def test_a_side_without_a_manifest_draws_nothing():
    rng = _CountingRandom(9)
    a = _augment(rng, noise=0, rirs=0)
    assert not a.active
    assert all(r == (-1, -1, 0.0, 0.0) for r in a.draw(10)) and rng.calls == 0
    one = _augment(rng, noise=0, rirs=2, rir_prob=0.0)
    assert one.active and all(r.rir == -1 and r.clip == -1 for r in one.draw(10)) and rng.calls == 10


# ---------------------------------------------------------------------------------------------------------------- config
def test_config_keys_parse_and_default_to_off():
    from wav2letter_pytorch_amd.data.augment_wave import from_config, parse_range
    from wav2letter_pytorch_amd.train import build_config
    cfg = build_config(['data.train_manifest=t.csv', 'data.noise_manifest=n.csv', 'data.snr_db=0,15', 'data.rir_prob=0.3'])
    assert cfg.data.noise_manifest == 'n.csv' and parse_range(cfg.data.snr_db) == (0.0, 15.0) and cfg.data.rir_prob == 0.3
    assert cfg.data.rir_manifest is None and cfg.data.noise_prob == 0.5 and cfg.data.rir_max_seconds == 0.5
    cfg = build_config([])
    assert cfg.data.noise_manifest is None and cfg.data.rir_manifest is None
    assert parse_range(cfg.data.snr_db) == (5.0, 20.0)
    assert from_config(cfg.data, 16000) is None          # both manifests None: no augmenter at all
    assert parse_range('5,20') == (5.0, 20.0) and parse_range([1, 2]) == (1.0, 2.0) and parse_range(7) == (7.0, 7.0)


def test_config_rejects_a_reversed_range_and_a_bad_probability():
    from wav2letter_pytorch_amd.data.augment_wave import WaveformAugment, parse_range
    from wav2letter_pytorch_amd.train import build_config
    with pytest.raises(ValueError):
        parse_range('20,5')
    with pytest.raises(ValueError):
        build_config(['data.snr_db=20,5'])
    with pytest.raises(ValueError):
        build_config(['data.noise_prob=1.5'])
    with pytest.raises(ValueError):
        build_config(['data.rir_prob=-0.1'])
    with pytest.raises(ValueError):
        WaveformAugment(noise_prob=2)
    with pytest.raises(ValueError):
        WaveformAugment(snr_db=(9, 1))


# ---------------------------------------------------------------------------------------------------------------- ABI
def test_header_declares_and_library_exports_the_entry_points():
    from wav2letter_pytorch_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'w2l_hip.h')).read()
    for name in ('w2l_reverb', 'w2l_mix_noise', 'w2l_mix_noise_slab_doubles'):
        assert re.search(r'\b%s\s*\(' % name, hdr), name
        assert name in _lib.EXPORTED_SYMBOLS and getattr(_lib.lib, name)
    assert _lib.lib.w2l_abi_version() == 2
    consts = dict(re.findall(r'#define (W2L_(?:REVERB|MIX)_\w+) (\d+)', hdr))
    assert int(consts['W2L_REVERB_MAX_TAPS']) == 16384 == __import__('wav2letter_pytorch_amd.data.augment_wave', fromlist=['x']).MAX_TAPS
    assert {'W2L_REVERB_TILE', 'W2L_REVERB_CHUNK', 'W2L_MIX_TILE'} <= set(consts)
    assert _lib.lib.w2l_mix_noise_slab_doubles(3, 2 * int(consts['W2L_MIX_TILE']) + 1) == 3 * 3 * 2


def test_argument_checks_need_no_gpu():
    """the host validates every descriptor before anything is launched: the refusals are reachable without a device"""
    from wav2letter_pytorch_amd._lib import lib
    rows = np.array([[10, 0]], dtype=np.int32)
    banks = np.array([[0, 16385, 0]], dtype=np.int32)
    fake = ctypes.c_void_p(4096)                         # never dereferenced: the call fails in the checks
    rc = lib.w2l_reverb(fake, 16, ctypes.c_void_p(8192), 16, 1, rows.ctypes.data, fake, banks.ctypes.data, fake, 1, fake, 20000, None)
    assert rc != 0 and b'16384' in lib.w2l_last_error()
