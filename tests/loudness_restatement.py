"""numpy restatement of Loudness (include/soundml_amd.h words the definitions, DESIGN.md 4.8l the orders), no GPU.  Every product
and every sum is its own numpy operation on float64 arrays, so nothing fuses; serial sums are np.cumsum, which adds left to right.

    k_weighting(rate), taps()            the two host-built tables by their formulas
    weighted(rate, x)                    the K-weighted signal: iir_restatement.stated over the two sections, float64 [rows; n]
    step_energies(rate, y)               pieces (Iir block x gating step) summed serially, then onto their step ascending
    window_energies(E, count, w, inv)    w steps ascending, times inv
    channel_sum(z, weights)              (G_0 z_0 + G_1 z_1) + ... ascending
    gates(e)                             the absolute and the relative gate on energies -> (abs mask, both mask, integrated)
    true_peak(x, h)                      the four phases, float64 sums in ascending j, max |y| per row
    gain(i, peaks, target, ceiling)      normalize's one gain per clip
    measure(x, rate, weights)            everything above for audio [clips; channels; n]
and the EBU Tech 3341 signals the tests share."""
import functools

import numpy as np

import iir_restatement as IR

BLOCK = IR.BLOCK
MIN_RATE = 8000
E_ABS = 10.0 ** ((-70.0 + 0.691) / 10.0)
SURROUND_5_0 = (1.0, 1.0, 1.0, 1.41, 1.41)


def k_weighting(rate):
    fs = float(rate)
    f0, G, Q = 1681.974450955533, 3.999843853973347, 0.7071752369554196
    K = np.tan(np.pi * f0 / fs)
    Vh = 10.0 ** (G / 20.0)
    Vb = Vh ** 0.4996667741545416
    a0 = 1.0 + K / Q + K * K
    shelf = [(Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0, 1.0, 2.0 * (K * K - 1.0) / a0,
             (1.0 - K / Q + K * K) / a0]
    f0, Q = 38.13547087602444, 0.5003270373238773
    K = np.tan(np.pi * f0 / fs)
    a0 = 1.0 + K / Q + K * K
    high = [1.0, -2.0, 1.0, 1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]
    return np.array([shelf, high], np.float64)


def taps():
    k = np.arange(49)
    h = np.sinc((k - 24) / 4.0) * np.kaiser(49, 8.0)
    return h * (4.0 / h.sum())


def step(rate):
    return (int(rate) + 5) // 10


def blocks(rate, n):
    s = step(rate)
    return 0 if n < 4 * s else (n - 4 * s) // s + 1


def weighted(rate, x, sos=None):
    """float64 [rows; n]: Iir's stated order from a zero state"""
    x = np.atleast_2d(np.asarray(x, np.float64))
    if x.shape[1] == 0:
        return x.copy()
    return IR.stated(k_weighting(rate) if sos is None else sos, x)


def step_energies(rate, y):
    """E [rows; n // step + 1]: entry k is the sum of the pieces of step k, each piece summed serially from its first sample, the
    pieces added ascending from 0; the last entry is the open step's closed pieces (no face reads it)"""
    rows, n = y.shape
    s = step(rate)
    E = np.zeros((rows, n // s + 1))
    cuts = sorted(set(range(0, n, BLOCK)) | set(range(0, n, s)) | {n})
    yy = y * y
    for a, b in zip(cuts[:-1], cuts[1:]):
        E[:, a // s] = E[:, a // s] + np.cumsum(yy[:, a:b], axis=1)[:, -1]
    return E


def window_energies(E, count, window, inv):
    """[rows; count]: (((E[j] + E[j+1]) + ...) + E[j+window-1]) inv"""
    if count <= 0:
        return np.zeros((E.shape[0], 0))
    acc = E[:, 0:count].copy()
    for i in range(1, window):
        acc = acc + E[:, i:i + count]
    return acc * inv


def channel_sum(z, weights=None):
    """z [clips; channels; nb] -> e [clips; nb]"""
    g = np.ones(z.shape[1]) if weights is None else np.asarray(weights, np.float64)
    e = g[0] * z[:, 0]
    for c in range(1, z.shape[1]):
        e = e + g[c] * z[:, c]
    return e


def lufs(e):
    with np.errstate(divide="ignore"):
        return -0.691 + 10.0 * np.log10(e)


def serial_mean(v):
    return np.cumsum(v)[-1] / float(v.size)


def gates(e):
    """e [nb] -> (through the absolute gate, through both, integrated loudness or -inf)"""
    e = np.asarray(e, np.float64)
    first = e > E_ABS
    if not first.any():
        return first, first.copy(), -np.inf
    relative = 0.1 * serial_mean(e[first])
    both = first & (e > relative)
    if not both.any():
        return first, both, -np.inf
    return first, both, float(lufs(serial_mean(e[both])))


def true_peak(x, h=None):
    """x [rows; n] -> max over i < n and the four phases of |sum_j h[p + 4 j] x[i - j]|, float64 [rows]"""
    h = taps() if h is None else np.asarray(h, np.float64)
    x = np.atleast_2d(np.asarray(x, np.float64))
    rows, n = x.shape
    peak = np.zeros(rows)
    if n == 0:
        return peak
    xp = np.concatenate([np.zeros((rows, 12)), x], axis=1)
    for p in range(4):
        acc = h[p] * xp[:, 12:12 + n]
        j = 1
        while p + 4 * j < 49:
            acc = acc + h[p + 4 * j] * xp[:, 12 - j:12 - j + n]
            j += 1
        peak = np.maximum(peak, np.abs(acc).max(axis=1))
    return peak


def gain(i, peaks, target=-23.0, ceiling=None):
    g = 1.0 if i == -np.inf else 10.0 ** ((target - i) / 20.0)
    if ceiling is not None:
        peak = float(np.max(peaks))
        if g * peak > ceiling:
            g = ceiling / peak
    return g


class Measured:
    pass


def measure(x, rate, weights=None):
    """x [clips; channels; n] -> the quantities of every face, float64"""
    x = np.asarray(x)
    clips, channels, n = x.shape
    s, nb = step(rate), blocks(rate, n)
    m = Measured()
    y = weighted(rate, x.reshape(clips * channels, n))
    m.E = step_energies(rate, y)
    m.z = window_energies(m.E, nb, 4, 1.0 / (4 * s)).reshape(clips, channels, nb)
    m.e = channel_sum(m.z, weights)
    m.momentary = lufs(m.e)
    st = window_energies(m.E, max(0, nb - 26), 30, 1.0 / (30 * s)).reshape(clips, channels, max(0, nb - 26))
    m.e_short = channel_sum(st, weights)
    m.short_term = lufs(m.e_short)
    g = [gates(m.e[c]) for c in range(clips)]
    m.mask = np.array([a.astype(np.uint8) | (b.astype(np.uint8) << 1) for a, b, _ in g], np.uint8).reshape(clips, nb)
    m.integrated = np.array([i for _, _, i in g], np.float64)
    return m


# ---- the shared signals -------------------------------------------------------------------------------------------------------

def sine(rate, seconds, dbfs, freq=1000.0, start=0):
    t = (start + np.arange(int(round(seconds * rate)))) / float(rate)
    return (10.0 ** (dbfs / 20.0)) * np.sin(2.0 * np.pi * freq * t)


# EBU Tech 3341 table 1, cases 1-6: (segments of (seconds, dBFS per channel), weights, expected LUFS); 1 kHz, 48 kHz
EBU = {
    1: ([(20.0, (-23.0, -23.0))], None, -23.0),
    2: ([(20.0, (-33.0, -33.0))], None, -33.0),
    3: ([(10.0, (-36.0, -36.0)), (60.0, (-23.0, -23.0)), (10.0, (-36.0, -36.0))], None, -23.0),
    4: ([(10.0, (-72.0, -72.0)), (10.0, (-36.0, -36.0)), (60.0, (-23.0, -23.0)), (10.0, (-36.0, -36.0)), (10.0, (-72.0, -72.0))], None, -23.0),
    5: ([(20.0, (-26.0, -26.0)), (20.1, (-20.0, -20.0)), (20.0, (-26.0, -26.0))], None, -23.0),
    6: ([(20.0, (-28.0, -28.0, -24.0, -30.0, -30.0))], SURROUND_5_0, -23.0),
}
EBU_RATE = 48000


@functools.lru_cache(maxsize=None)
def ebu_signal(case):
    """float32 [channels; n], the phase continuous across the segments"""
    segments, _, _ = EBU[case]
    parts, start = [], 0
    for seconds, levels in segments:
        parts.append(np.stack([sine(EBU_RATE, seconds, db, start=start) for db in levels]))
        start += parts[-1].shape[1]
    x = np.concatenate(parts, axis=1).astype(np.float32)
    x.setflags(write=False)
    return x


# the true-peak tones of EBU Tech 3341 cases 15-19: (cycles per sample, phase in degrees, amplitude, expected dBTP)
TONES = [(1 / 4, 0.0, 0.5, -6.0), (1 / 4, 45.0, 0.5, -6.0), (1 / 6, 60.0, 0.5, -6.0), (1 / 8, 67.5, 0.5, -6.0), (1 / 4, 45.0, 1.41, 3.0)]


@functools.lru_cache(maxsize=None)
def tone(k):
    """float32 [4800] under a 480-sample raised-cosine fade at each end (an unfaded onset measures the edge, not the filter)"""
    f, phase, amp, _ = TONES[k]
    i = np.arange(4800)
    x = amp * np.sin(2.0 * np.pi * f * i + np.deg2rad(phase))
    fade = 0.5 - 0.5 * np.cos(np.pi * (np.arange(480) + 0.5) / 480.0)
    x[:480] *= fade
    x[-480:] *= fade[::-1]
    x = x.astype(np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def noise(seed, clips, channels, n, scale=0.1):
    x = (scale * np.random.default_rng(seed).standard_normal((clips, channels, n))).astype(np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def measured_noise(seed, clips, channels, n, rate, scale=0.1):
    return measure(noise(seed, clips, channels, n, scale), rate)


@functools.lru_cache(maxsize=None)
def gating_clip():
    """3 s of stereo noise at 48 kHz in three levels: loud, 25 dB lower, 1e-5: the relative gate drops the middle blocks, the
    absolute gate the last ones (the test checks both, and the margins, by this restatement)"""
    rng = np.random.default_rng(77)
    n = 3 * 48000
    x = rng.standard_normal((1, 2, n))
    level = np.concatenate([np.full(48000, 0.1), np.full(48000, 0.1 * 10.0 ** (-25.0 / 20.0)), np.full(48000, 1e-5)])
    x = (x * level).astype(np.float32)
    x.setflags(write=False)
    return x
