"""Plain-numpy restatement of the reference's spectral contrast and onset strength (soundml/lib/contrast.ml, onset.ml) on top
of oracle.soundml_oracle, the yardstick of the contrast / onset tests.  A test helper, not part of the product: written from
the modules' documented semantics (the band plan, one sort and two means per band, the lagged positive difference, the shift).

test_contrast_onset_restatement.py pins it to the reference's own golden vectors (tests/golden/onset).
"""
import math

import numpy as np

from oracle import soundml_oracle as O

SEED = 20260802          # onset_goldens.ml:34


class Rejected(ValueError):
    """an Invalid_argument of the reference; str(e) is its message without the function's name"""


def rint(x):
    """Nearest integer, ties to even (contrast.ml:52-58)."""
    fl = math.floor(x)
    d = x - fl
    if d > 0.5:
        return fl + 1.0
    if d < 0.5:
        return fl
    return fl if math.fmod(fl, 2.0) == 0.0 else fl + 1.0


def plan(n_bands, f_min, quantile, sample_rate, fft_size):
    """contrast.ml:60-142: [(lo, sub_len, take)] for bands 0 .. n_bands, the checks in the reference's order."""
    if n_bands < 1:
        raise Rejected("cannot divide the spectrum into %d octave bands (n_bands must be at least 1)" % n_bands)
    if not (math.isfinite(f_min) and f_min > 0.0):
        raise Rejected("cannot start the first octave band at %g Hz (f_min must be finite and positive)" % f_min)
    if not (0.0 < quantile < 1.0):
        raise Rejected("cannot average the %g quantile of each band (quantile must lie strictly between 0 and 1)" % quantile)
    if sample_rate < 1:
        raise Rejected("cannot use a sample rate of %d Hz (sample_rate must be at least 1)" % sample_rate)

    def edge(j):
        return 0.0 if j == 0 else f_min * math.pow(2.0, float(j - 1))
    nyquist = 0.5 * float(sample_rate)
    if edge(n_bands) >= nyquist:
        raise Rejected("cannot start the top octave band at %g Hz at a sample rate of %d Hz (every band must start below the "
                       "Nyquist frequency %g; lower f_min or n_bands)" % (edge(n_bands), sample_rate, nyquist))
    bins = fft_size // 2 + 1
    step = 1.0 / (float(fft_size) * (1.0 / float(sample_rate)))
    f = np.arange(bins, dtype=np.float64) * step
    bands = []
    for k in range(n_bands + 1):
        f_low, f_high = edge(k), edge(k + 1)
        inside = np.nonzero((f >= f_low) & (f <= f_high))[0]
        where = "[%g, %g] Hz with an FFT of size %d at a sample rate of %d Hz" % (f_low, f_high, fft_size, sample_rate)
        if inside.size == 0:
            raise Rejected("cannot resolve the octave band %s (the band spans no FFT bin; raise fft_size or lower n_bands)" % where)
        lo0, hi0 = int(inside[0]), int(inside[-1])
        lo = lo0 - 1 if k > 0 else lo0
        hi = bins - 1 if k == n_bands else hi0
        count = hi - lo + 1
        take = max(1, int(rint(quantile * float(count))))
        sub_len = (hi if k == n_bands else hi - 1) - lo + 1
        if sub_len < 1:
            raise Rejected("cannot resolve the octave band %s (the band spans no FFT bin below its top edge; raise fft_size or "
                           "lower n_bands)" % where)
        bands.append((lo, sub_len, min(take, sub_len)))
    return bands


def means(s, bands):
    """(valley, peak) [...; n_bands + 1; frames] float64: the mean of the `take` smallest and largest magnitudes of each band"""
    s64 = np.asarray(s).astype(np.float64)
    valleys, peaks = [], []
    for lo, sub_len, take in bands:
        ordered = np.sort(s64[..., lo:lo + sub_len, :], axis=-2)
        valleys.append(np.mean(ordered[..., :take, :], axis=-2, keepdims=True))
        peaks.append(np.mean(ordered[..., sub_len - take:, :], axis=-2, keepdims=True))
    return np.concatenate(valleys, axis=-2), np.concatenate(peaks, axis=-2)


def contrast64(s, bands, linear=False, clamped=True):
    """contrast.ml:155-206 before the one rounding: float64 whatever the dtype of s"""
    s = np.asarray(s)
    if 0 in s.shape:
        return np.zeros(s.shape[:-2] + (len(bands), s.shape[-1]), np.float64)
    valley, peak = means(s, bands)
    if linear:
        return peak - valley
    top_db = 80.0 if clamped else None
    return O.power_to_db(peak, top_db=top_db) - O.power_to_db(valley, top_db=top_db)


def spectral_contrast_of_spectrogram(s, sample_rate, n_bands=6, f_min=200.0, quantile=0.02, linear=False, clamped=True, fft_size=None):
    s = np.asarray(s)
    fft_size = 2 * (s.shape[-2] - 1) if fft_size is None else fft_size
    return contrast64(s, plan(n_bands, f_min, quantile, sample_rate, fft_size), linear, clamped).astype(s.dtype)


def spectral_contrast(c, x, sample_rate, n_bands=6, f_min=200.0, quantile=0.02, linear=False):
    """contrast.ml:208-218 over the oracle's magnitude spectrogram"""
    bands = plan(n_bands, f_min, quantile, sample_rate, c.fft_size)
    s = O.power_spectrum(c, np.asarray(x), 1.0)
    return contrast64(s, bands, linear, True).astype(s.dtype)


def flux64(db, lag):
    """onset.ml:73-122 on one chunk with an empty carry, before the rounding: [...; bins; frames] -> [...; frames] float64"""
    db = np.asarray(db).astype(np.float64)
    frames = db.shape[-1]
    z = np.zeros(db.shape[:-2] + (frames,), np.float64)
    if frames > lag:
        z[..., lag:] = np.mean(np.maximum(db[..., lag:] - db[..., :frames - lag], 0.0), axis=-2)
    return z


def shift_of(c):
    return c.fft_size // (2 * c.hop) if c.alignment == "centered" else 0


def envelope64(mel, lag, shift):
    """onset.ml:170-198 from the mel spectrogram on, before the rounding"""
    mel = np.asarray(mel)
    frames = mel.shape[-1]
    if mel.size == 0:
        return np.zeros(mel.shape[:-2] + (frames,), np.float64)
    z = flux64(O.power_to_db(mel.astype(np.float64), top_db=80.0), lag)
    if shift == 0:
        return z
    out = np.zeros_like(z)
    if shift < frames:
        out[..., shift:] = z[..., :frames - shift]
    return out


def onset_strength(c, mc, x, lag=1):
    x = np.asarray(x)
    mel = O.mel_spectrogram(c, mc, x)
    return envelope64(mel, lag, shift_of(c)).astype(mel.dtype)


def signal(n, envelope=False, silence_tail=False):
    """onset_goldens.ml:36-46: the suite's LCG signal, optionally shaped by exp(-12 i / n), the second half zeroed"""
    x = O.lcg_signal(n, SEED, envelope=envelope)
    if silence_tail:
        x[n // 2:] = 0.0
    return x


def ulp32(want64):
    """the spacing of float32 at each value of want64 (at least the smallest normal's)"""
    a = np.maximum(np.abs(np.asarray(want64, np.float64)), float(np.finfo(np.float32).tiny)).astype(np.float32)
    return np.spacing(a).astype(np.float64)


def within_ulp32(got, want64, absolute=0.0):
    """|got - want64| <= ulp_float32(want64) + absolute, elementwise; returns the worst excess (<= 0 passes)"""
    got = np.asarray(got).astype(np.float64)
    assert got.shape == np.asarray(want64).shape, (got.shape, np.asarray(want64).shape)
    if got.size == 0:
        return 0.0
    return float(np.max(np.abs(got - want64) - (ulp32(want64) + absolute)))
