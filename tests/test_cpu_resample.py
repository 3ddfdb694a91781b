"""The host side of the sample-rate converter (data/resample.py), no GPU: the filter bank against the float64 formula, ratio
reduction and output lengths, the speed-perturbation draw, the bank-size cap, and the QUALITY of the definition itself --
the float64 reference run with the fp32 bank on pure tones: error against the analytically resampled tone in the passband,
residual level of tones above the output Nyquist.  The gate is -80 dB (the definition measures about -93 dB; a shorter test
signal than the one it was measured on costs a few dB)."""
import math
import os
import random
import sys
from fractions import Fraction

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resample_refs as RR  # noqa: E402

RATIOS = [(3, 1), (441, 160), (1, 2), (9, 10), (11, 10)]
OUT_RATE = 16000
GATE_DB = -80.0
EDGE = 300                       # output samples left out at each end (the filter's reach into the zero padding)

_BANKS = {}


def _bank(P, Q):
    from wav2letter_pytorch_amd.data.resample import filter_bank
    if (P, Q) not in _BANKS:
        _BANKS[P, Q] = filter_bank(P, Q)
    return _BANKS[P, Q]


def test_module_imports_without_a_device_and_states_the_defaults():
    from wav2letter_pytorch_amd.data import resample as R
    assert (R.ZEROS, R.BETA, R.ROLLOFF) == (16, 9.0, 0.92)
    assert R.MAX_BANK_BYTES == 8 << 20


@pytest.mark.parametrize('P,Q', RATIOS + [(4851, 1600)])
def test_filter_bank_is_the_float64_formula_rounded_once(P, Q):
    h, H = _bank(P, Q)
    phases = list(range(Q)) if Q <= 160 else sorted({0, 1, Q // 2, Q - 1} | set(range(3, Q, 53)))    # every row of the small banks
    want, want_h = RR.bank_ref(P, Q, phases=phases)
    assert H == want_h and h.dtype == np.float32 and h.shape == want.shape == (Q, 2 * H + 2)
    np.testing.assert_array_equal(h[phases], want[phases].astype(np.float32))


def test_bank_shapes_and_sizes_of_the_common_ratios():
    from wav2letter_pytorch_amd.data.resample import bank_shape
    assert bank_shape(3, 1) == (108, 53)                 # 48 k -> 16 k
    assert bank_shape(9, 10) == (38, 18)                 # speed 0.9
    K, _ = bank_shape(441, 160)
    assert 160 * K * 4 // 1024 == 61                     # 61 KB
    K, _ = bank_shape(4851, 1600)
    assert 1600 * K * 4 // 1024 == 675                   # 44.1 k -> 16 k at speed 1.1: 675 KB


@pytest.mark.parametrize('file_rate,speed,want,n_in,n_out', [
    (48000, 1, Fraction(3, 1), 4099, 1367),
    (8000, 1, Fraction(1, 2), 1537, 3074),
    (44100, 1, Fraction(441, 160), 10007, 3631),
    (16000, 0.9, Fraction(9, 10), 7, 8),
    (16000, 1.1, Fraction(11, 10), 3001, 2729),
    (16000, 1.0, Fraction(1, 1), 2500, 2500),
    (44100, 1.1, Fraction(4851, 1600), 3000017, 989493),
])
def test_ratio_reduction_and_output_length(file_rate, speed, want, n_in, n_out):
    from wav2letter_pytorch_amd.data.resample import output_length, resample_ratio
    r = resample_ratio(file_rate, OUT_RATE, speed)
    assert isinstance(r, Fraction) and r == want
    assert n_out == math.ceil(Fraction(n_in) / want)     # the table's own figure, in exact rationals
    assert output_length(n_in, r) == n_out == RR.n_out_ref(n_in, want.numerator, want.denominator)


def test_speed_factors_become_exact_small_ratios():
    from wav2letter_pytorch_amd.data.resample import resample_ratio, speed_fraction
    assert speed_fraction(0.9) == Fraction(9, 10) and speed_fraction(1.1) == Fraction(11, 10) and speed_fraction(1) == 1
    assert speed_fraction(np.float64(1.05)) == Fraction(21, 20)
    assert speed_fraction(1 / 3).denominator <= 1000
    assert resample_ratio(16000, 16000) == 1 and resample_ratio(22050, 16000) == Fraction(441, 320)
    with pytest.raises(ValueError):
        resample_ratio(0, 16000)


def test_speed_perturb_is_reproducible_and_stays_in_its_list():
    from wav2letter_pytorch_amd.data.resample import SpeedPerturb
    a = SpeedPerturb(rng=random.Random(5)).draw(200)
    b = SpeedPerturb((0.9, 1.0, 1.1), rng=random.Random(5)).draw(200)
    assert a == b and set(a) == {0.9, 1.0, 1.1}
    assert SpeedPerturb(rng=random.Random(6)).draw(200) != a
    one = SpeedPerturb((1.05,), rng=random.Random(0))
    assert one(7) == [1.05] * 7
    with pytest.raises(ValueError):
        SpeedPerturb(())
    with pytest.raises(ValueError):
        SpeedPerturb((0.9, 0.0))


def test_speed_factor_config_forms():
    from wav2letter_pytorch_amd.data.resample import parse_speed_factors
    assert parse_speed_factors('0.9,1.0,1.1') == (0.9, 1.0, 1.1) == parse_speed_factors([0.9, 1.0, 1.1])
    assert parse_speed_factors(None) is None and parse_speed_factors('null') is None and parse_speed_factors(1.1) == (1.1,)
    from wav2letter_pytorch_amd.train import build_config
    cfg = build_config(['data.resample=true', 'data.speed_perturb=0.9,1.0,1.1'])
    assert cfg.data.resample is True and parse_speed_factors(cfg.data.speed_perturb) == (0.9, 1.0, 1.1)
    cfg = build_config([])
    assert cfg.data.resample is False and cfg.data.speed_perturb is None


def test_bank_size_cap_names_the_ratio():
    from wav2letter_pytorch_amd.data.resample import BankCache, filter_bank, resample_ratio
    r = resample_ratio(44100, 16000, 1.001)              # 441441/160000: 160000 phases x 98 taps = 63 MB
    with pytest.raises(ValueError, match=f'{r.numerator}/{r.denominator}'):
        filter_bank(r.numerator, r.denominator)
    with pytest.raises(ValueError, match='441441/160000'):
        BankCache().bank(r.numerator, r.denominator)
    with pytest.raises(ValueError, match='20/1'):        # 320 k -> 16 k: more taps per output than the kernel supports
        BankCache().bank(20, 1)
    cache = BankCache()
    assert cache.bank(3, 1) == 0 and cache.bank(9, 10) == 1 and cache.bank(3, 1) == 0
    np.testing.assert_array_equal(cache.desc, [[0, 108, 53, 1], [108, 38, 18, 10]])


def _db(num, den):
    return 10.0 * math.log10(max(float(np.mean(num ** 2)), 1e-300) / float(np.mean(den ** 2)))


def _tone_through(P, Q, f_hz):
    """0.5 s of a unit sine at f_hz, sampled at OUT_RATE * P / Q, through the float64 reference with the fp32 bank; returns
    (output, the same tone sampled at OUT_RATE) without the EDGE samples at either end"""
    in_rate = Fraction(OUT_RATE * P, Q)
    n_in = int(in_rate / 2)
    x = np.sin(2.0 * np.pi * (f_hz / float(in_rate)) * np.arange(n_in, dtype=np.float64))
    h, _ = _bank(P, Q)
    got, _ = RR.resample_ref(x, P, Q, h)
    want = np.sin(2.0 * np.pi * (f_hz / OUT_RATE) * np.arange(got.shape[0], dtype=np.float64))
    assert got.shape[0] > 4 * EDGE
    return got[EDGE:-EDGE], want[EDGE:-EDGE]


@pytest.mark.parametrize('P,Q', RATIOS)
@pytest.mark.parametrize('frac', [0.1, 0.5, 0.75])
def test_passband_error_against_the_analytic_tone(P, Q, frac):
    """tones at 0.1 / 0.5 / 0.75 of the lower of the two Nyquist frequencies: error power over tone power <= -80 dB, and the
    largest single error as well"""
    nyq = min(OUT_RATE, OUT_RATE * P / Q) / 2
    got, want = _tone_through(P, Q, frac * nyq)
    err_db = _db(got - want, want)
    peak_db = 20.0 * math.log10(np.abs(got - want).max())
    print(f'{P}/{Q} tone at {frac} Nyquist: error {err_db:.1f} dB rms, {peak_db:.1f} dB peak')
    assert err_db <= GATE_DB and peak_db <= GATE_DB


@pytest.mark.parametrize('P,Q', [(3, 1), (441, 160)])
@pytest.mark.parametrize('frac', [1.1, 1.5])
def test_tones_above_the_output_nyquist_are_removed(P, Q, frac):
    got, want = _tone_through(P, Q, frac * OUT_RATE / 2)
    level_db = _db(got, np.full(1, math.sqrt(0.5)))       # against the power of a unit sine
    print(f'{P}/{Q} tone at {frac} of the output Nyquist: residual {level_db:.1f} dB')
    assert level_db <= GATE_DB


def test_reference_copies_nothing_and_reaches_into_zero_padding():
    """properties of the restated reference itself: DC gain of every phase within the passband ripple, and a row shorter
    than the filter's reach uses zeros outside [0, n_in)"""
    h, H = _bank(9, 10)
    assert np.abs(h.astype(np.float64).sum(axis=1) - 1.0).max() < 1e-4
    x = np.arange(1, 8, dtype=np.float64)
    got, A = RR.resample_ref(x, 9, 10, h)
    assert got.shape == (8,) and (A >= np.abs(got)).all()
    want0 = sum(x[i] * float(h[0, H + i]) for i in range(7))          # m = 0: i0 = 0, phase 0, taps H .. H + 6 meet x[0 .. 6]
    assert abs(got[0] - want0) < 1e-12
