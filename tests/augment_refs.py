"""Float64 restatements of the waveform augmentations, written from their definitions -- plain NumPy, nothing of the package:

    reverb:   out[m] = sum_{j < K} h[j] x~[m + d - j],  0 <= m < n_in,  x~ = 0 outside [0, n_in)
    mix:      Ps = mean_{m < n_in} x[m]^2,  Pz = mean_{m < n_in} z[(o + m) mod n_z]^2,  g = sqrt(Ps / (Pz 10^(snr_db / 10))),
              out[m] = x[m] + g z[(o + m) mod n_z];  a row with Ps = 0 or Pz = 0 is returned unchanged
    prepare:  mono -> p = argmax |h| -> h[0 : p + int(max_seconds rate)] -> d = p -> sum h^2 = 1 in float64 -> fp32 once
"""
import numpy as np


def reverb_ref(x, h, d):
    """(out float64 [n_in], A float64 [n_in]) with A[m] = sum_j |h[j]| |x~[m + d - j]|, the scale of the rounding bound"""
    x = np.asarray(x, dtype=np.float64)
    h = np.asarray(h, dtype=np.float64)
    n, K = x.shape[0], h.shape[0]
    assert 0 <= d < K
    out = np.zeros(n, dtype=np.float64)
    A = np.zeros(n, dtype=np.float64)
    ax, ah = np.abs(x), np.abs(h)
    for j in range(K):                                   # out[m] += h[j] x[m + d - j] for the m with 0 <= m + d - j < n
        lo, hi = max(0, j - d), min(n, n + j - d)
        if lo < hi:
            out[lo:hi] += h[j] * x[lo + d - j:hi + d - j]
            A[lo:hi] += ah[j] * ax[lo + d - j:hi + d - j]
    return out, A


def reverb_bound(A, K):
    """the fmaf-chain bound: K products in a few separately accumulated chains"""
    return 1.01 * (K + 64) * 2.0 ** -24 * np.asarray(A, dtype=np.float64) + 1e-30


def mix_ref(x, z, o, snr_db):
    """(out float64 [n_in], g, wrapped clip float64 [n_in]); g = 0 where the row is returned unchanged"""
    x = np.asarray(x, dtype=np.float64)
    z = np.asarray(z, dtype=np.float64)
    n, n_z = x.shape[0], z.shape[0]
    if n_z == 0 or n == 0:
        return x.copy(), 0.0, np.zeros(n)
    assert 0 <= o < n_z
    zw = z[(o + np.arange(n, dtype=np.int64)) % n_z]
    ps, pz = np.mean(x * x), np.mean(zw * zw)
    if ps == 0.0 or pz == 0.0:
        return x.copy(), 0.0, zw
    g = float(np.sqrt(ps / (pz * 10.0 ** (float(snr_db) / 10.0))))
    return x + g * zw, g, zw


def snr_db_of(x, out):
    """the SNR in dB of ``out`` = x + noise, measured over the row"""
    x = np.asarray(x, dtype=np.float64)
    e = np.asarray(out, dtype=np.float64) - x
    return 10.0 * np.log10(np.mean(x * x) / np.mean(e * e))


def prepare_rir_ref(samples, rate, max_seconds=0.5):
    """(h float32 [K], d) of a response already at the model's rate"""
    h = np.asarray(samples, dtype=np.float64)
    if h.ndim > 1:
        h = h.mean(axis=1)
    p = int(np.argmax(np.abs(h)))
    h = h[:p + int(max_seconds * rate)]
    h = h / np.sqrt(np.sum(h * h))
    return h.astype(np.float32), p
