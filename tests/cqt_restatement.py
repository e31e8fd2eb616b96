"""A numpy float64 restatement of the reference's constant-Q / variable-Q module (soundml/lib/cqt.ml) and of the 0/1 fold of
chroma.ml:332-385, in the reference's own order: the plan of ``Config.create`` (cqt.ml:121-424), then per octave a
rectangular centered STFT (``np.fft.rfft`` of the framed signal) and ``K @ D`` with the half-spectrum filter matrix
(cqt.ml:615-667).  The 2:1 decimator is passed in as a callable, so one restatement serves the CPU pin on the goldens
(tests/test_cqt_restatement.py: the sparse polyphase stage of effects_restatement) and the composition tests on the device
(tests/test_gpu_cqt.py: the library's own ``Resample.apply``, so both sides project the same octave signals).
"""
import json
import math
import os
import sys

import numpy as np

from oracle import soundml_oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# cqt_goldens.ml:27-47: fractions of the case peak max|expected|, plus rtol
TIGHT_ATOL, TIGHT32_ATOL, WIDE_ATOL, RTOL = 1e-6, 5e-6, 6e-4, 1e-5
# chroma_goldens.ml:35-39
CHROMA_CQT_ATOL, CHROMA_CQT_ODD_HOP_ATOL, CHROMA_CQT_RTOL = 1e-4, 1e-6, 1e-5
SEED = 20260803   # cqt_goldens.ml:49

C1 = 32.70319566257483

# cqt.ml:36-52: the tabulated equivalent noise bandwidths, in FFT bins
ENBW = {"hann": 1.50018310546875, "hamming": 1.3629455320350348, "blackman": 1.7269681554262326,
        "blackman_harris": 2.0045975283585014, "nuttall": 1.9763500280946082, "bartlett": 1.3334961334912805,
        "flat_top": 2.7762255046484143, "rectangular": 1.0}


def golden_cases(suite, name):
    """The cases of a reference vector file, each {"name", "params", "shape", "values"}.  The cqt files and chroma_cqt are
    committed repacked, values untouched: <name>.cases.json holds every case's name, parameters and shape, <name>.npz its
    float64 values under the case's name."""
    packed = os.path.join(GOLDEN, suite, name + ".cases.json")
    if not os.path.exists(packed):
        with open(os.path.join(GOLDEN, suite, name + ".json")) as fh:
            return json.load(fh)["cases"]
    with open(packed) as fh:
        cases = json.load(fh)["cases"]
    values = np.load(os.path.join(GOLDEN, suite, name + ".npz"))
    return [dict(c, values=values[c["name"]].tolist()) for c in cases]


def golden_signal(params):
    """cqt_goldens.ml:51-84, 163-190: the LCG under this suite's seed or the harmonic recipe, float64."""
    n = params["length"]
    if params["signal"] == "lcg":
        return O.lcg_signal(n, SEED)
    return O.harmonic_signal(n, params["sample_rate"], SEED)


def golden_kwargs(params):
    """The arguments of ``Config.create`` a golden case names (cqt_goldens.ml:94-159), defaults elsewhere."""
    kw = dict(n_bins=params["n_bins"], sample_rate=params["sample_rate"], fmin=params["fmin"],
              bins_per_octave=params["bins_per_octave"], tuning=params["tuning"])
    gamma = params.get("gamma")
    if gamma is not None:
        kw["gamma"] = "erb" if gamma == "erb" else ("constant_q" if gamma == "0.0" else float(gamma))
    window = params.get("window")
    if window is not None:
        kw["window"] = {"hann": "hann", "blackmanharris": "blackman_harris"}.get(window) or ("kaiser", params["beta"])
    for key in ("filter_scale", "hop", "scale"):
        if key in params:
            kw[key] = params[key]
    return kw


def _g(v):
    return "%g" % v


def window_parts(window):
    return (window, None) if isinstance(window, str) else (window[0], float(window[1]))


def enbw(window):
    """cqt.ml:31-54: the table, else n * sum w^2 / (sum w)^2 measured on 1000 periodic points."""
    kind, param = window_parts(window)
    if kind in ENBW:
        return ENBW[kind]
    w = O.window(kind, 1000, True, param)
    total = float(np.sum(w))
    return 1000.0 * float(np.sum(w * w)) / (total * total)


def two_factors(x):
    n = 0
    while x > 0 and x % 2 == 0:
        n, x = n + 1, x // 2
    return n


def next_power_of_two(x):
    return int(math.pow(2.0, float(int(math.ceil(math.log2(x))))))


def centre_frequencies(fmin, tuning, bins_per_octave, n_bins):   # cqt.ml:121-131
    anchor = fmin * math.pow(2.0, tuning / float(bins_per_octave))
    ratios = [math.pow(2.0, float(j) / float(bins_per_octave)) for j in range(bins_per_octave)]
    return np.array([math.pow(2.0, float(k // bins_per_octave)) * ratios[k % bins_per_octave] * anchor for k in range(n_bins)])


def relative_bandwidths(freqs):   # cqt.ml:140-153
    n = len(freqs)
    logf = [math.log2(f) for f in freqs]
    out = []
    for k in range(n):
        if k == 0:
            b = 1.0 / (logf[1] - logf[0])
        elif k == n - 1:
            b = 1.0 / (logf[n - 1] - logf[n - 2])
        else:
            b = 2.0 / (logf[k + 1] - logf[k - 1])
        r = math.pow(2.0, 2.0 / b)
        out.append((r - 1.0) / (r + 1.0))
    return np.array(out)


def filter_lengths_at(filter_scale, freqs, alphas, gammas, sample_rate):   # cqt.ml:174-177
    return np.array([(filter_scale / a) * sample_rate / (f + g / a) for f, a, g in zip(freqs, alphas, gammas)])


def octave_basis(window, norm, lengths, freqs, sample_rate, n_fft):
    """cqt.ml:202-246 up to the transform: the [count; n_fft] complex time-domain filters."""
    kind, param = window_parts(window)
    basis = np.zeros((len(freqs), n_fft), dtype=np.complex128)
    for j, length in enumerate(lengths):
        first, last = int(math.floor(-length / 2.0)), int(math.floor(length / 2.0))
        count = last - first
        w = O.window(kind, count, True, param)
        t = np.arange(first, last, dtype=np.float64)
        angle = t * 2.0 * math.pi * freqs[j] / sample_rate
        real, imag = np.cos(angle) * w, np.sin(angle) * w
        modulus = np.hypot(real, imag)
        mass = float(np.sum(modulus)) if norm == 1.0 else math.pow(float(np.sum(modulus ** norm)), 1.0 / norm)
        if mass < sys.float_info.min:
            mass = 1.0
        rescale = length / float(n_fft)
        left = (n_fft - count) // 2
        basis[j, left:left + count] = (real / mass * rescale) + 1j * (imag / mass * rescale)
    return basis


class Octave:
    def __init__(self, first, count, n_fft, hop, halvings, kernel):
        self.first, self.count, self.n_fft, self.hop, self.halvings, self.kernel = first, count, n_fft, hop, halvings, kernel

    def taps(self):
        """The kernel's time-domain form: g[b, n] = sum_{k <= n_fft / 2} K[b, k] exp(-2 pi i k n / n_fft), so that
        K @ rfft(frame) = sum_n frame[n] g[b, n]."""
        z = np.zeros((self.count, self.n_fft), dtype=np.complex128)
        z[:, :self.n_fft // 2 + 1] = self.kernel
        return np.fft.fft(z, axis=1)


class Config:
    """``Cqt.Config.create`` (cqt.ml:287-424); raises ValueError with the reference's message."""

    def __init__(self, n_bins, sample_rate, fmin=C1, bins_per_octave=12, gamma="constant_q", tuning=0.0, filter_scale=1.0,
                 norm=1.0, window="hann", scale=True, hop=512, pad="constant", pad_value=0.0):
        for name, value, floor in (("n_bins", n_bins, 1), ("bins_per_octave", bins_per_octave, 1), ("hop", hop, 1),
                                   ("sample_rate", sample_rate, 1)):
            if value < floor:
                raise ValueError("create: cannot use %s = %d (%s must be at least %d)" % (name, value, name, floor))
        positive = lambda v: v > 0.0
        for name, value, ok, text in (("fmin", fmin, positive, "finite and positive"), ("tuning", tuning, lambda v: True, "finite"),
                                      ("filter_scale", filter_scale, positive, "finite and positive"),
                                      ("norm", norm, positive, "finite and positive")):
            if not (math.isfinite(value) and ok(value)):
                raise ValueError("create: cannot use %s = %s (%s must be %s)" % (name, _g(value), name, text))
        if not isinstance(gamma, str) and not (math.isfinite(gamma) and gamma >= 0.0):
            raise ValueError("create: cannot use gamma = %s (gamma must be finite and non-negative)" % _g(gamma))
        try:
            bandwidth = enbw(window)
        except ValueError as e:   # cqt.ml:273-285 relabel_window
            raise ValueError("create" + str(e)[str(e).index(":"):])
        self.n_bins, self.sample_rate, self.fmin, self.bins_per_octave, self.gamma = n_bins, sample_rate, fmin, bins_per_octave, gamma
        self.tuning, self.filter_scale, self.norm, self.window, self.scale, self.hop = tuning, filter_scale, norm, window, scale, hop
        self.pad, self.pad_value = pad, pad_value
        with np.errstate(over="ignore"):
            try:
                freqs = centre_frequencies(fmin, tuning, bins_per_octave, n_bins)
            except OverflowError:
                freqs = np.array([math.inf])
        if not np.all(np.isfinite(freqs)):
            raise ValueError("create: cannot place %d bins from %s Hz at %d bins per octave (the frequency ladder overflows)"
                             % (n_bins, _g(fmin), bins_per_octave))
        if n_bins == 1:   # cqt.ml:157-159
            r = math.pow(2.0, 1.0 / float(bins_per_octave))
            alphas = np.array([((r * r) - 1.0) / ((r * r) + 1.0)])
        else:
            alphas = relative_bandwidths(freqs)
        if gamma == "constant_q":
            gammas = np.zeros(n_bins)
        elif gamma == "erb":
            gammas = alphas * 24.7 / 0.108
        else:
            gammas = np.full(n_bins, float(gamma))
        sr = float(sample_rate)
        self.freqs, self.alphas, self.gammas = freqs, alphas, gammas
        self.lengths = filter_lengths_at(filter_scale, freqs, alphas, gammas, sr)
        bound, limit = -math.inf, 0   # cqt.ml:183-193
        for k in range(n_bins):
            q = filter_scale / alphas[k]
            v = (freqs[k] * (1.0 + (0.5 * bandwidth / q))) + (0.5 * gammas[k])
            if v > bound:
                bound, limit = v, k
        self.cutoff = bound
        nyquist = sr / 2.0
        if bound > nyquist:
            raise ValueError("create: cannot place %d bins from %s Hz at a sample rate of %d Hz (bin %d, centred at %s Hz, "
                             "reaches %s Hz, above the Nyquist frequency %s)"
                             % (n_bins, _g(fmin), sample_rate, limit, _g(freqs[limit]), _g(bound), _g(nyquist)))
        self.n_octaves = -(-n_bins // bins_per_octave)
        n_filters = min(bins_per_octave, n_bins)
        head = max(0, int(math.ceil(math.log2(nyquist / bound))) - 2)
        tail = max(0, two_factors(hop) - self.n_octaves + 1)
        self.early = min(head, tail)
        self.base_rate = sr / float(1 << self.early)
        rate, octave_hop, halved = self.base_rate, hop // (1 << self.early), 0
        self.octaves = []
        for i in range(self.n_octaves):
            first = max(0, n_bins - (n_filters * (i + 1)))
            count = n_bins - (n_filters * i) - first
            sel = slice(first, first + count)
            lengths = filter_lengths_at(filter_scale, freqs[sel], alphas[sel], gammas[sel], rate)
            n_fft = next_power_of_two(float(np.max(np.maximum(lengths, 0.0))))
            if n_fft < 1:
                raise ValueError("create: cannot resolve %d bins from %s Hz with filter_scale = %s (the filters of octave %d "
                                 "span less than one sample)" % (n_bins, _g(fmin), _g(filter_scale), i))
            basis = octave_basis(window, norm, lengths, freqs[sel], rate, n_fft)
            kernel = np.fft.fft(basis, axis=1)[:, :n_fft // 2 + 1] * math.sqrt(self.base_rate / rate)
            self.octaves.append(Octave(first, count, n_fft, octave_hop, halved, kernel))
            if octave_hop % 2 == 0:
                octave_hop, rate, halved = octave_hop // 2, rate / 2.0, halved + 1
        self.divisors = np.sqrt(filter_lengths_at(filter_scale, freqs, alphas, gammas, self.base_rate)) if scale else None

    def latency(self, k):
        """cqt.ml:471-479 with ``k`` the group delay of the 2:1 plan: max over octaves of D (L - 1) + K (D - 1) + 1."""
        return max((1 << (self.early + o.halvings)) * (o.n_fft // 2 - 1) + k * ((1 << (self.early + o.halvings)) - 1) + 1
                   for o in self.octaves)


def stft_frames(n_fft, hop, n):
    """Stft.frames of the centered analysis (stft.ml:217-223)."""
    if n == 0:
        return 0
    padded = n + 2 * (n_fft // 2)
    return 0 if padded < n_fft else 1 + (padded - n_fft) // hop


def frames(c, n):   # cqt.ml:543-556
    if n < 0:
        raise ValueError("frames: cannot analyse a signal of length %d (length must be non-negative)" % n)
    return min(stft_frames(o.n_fft, o.hop, -(-n // (1 << (c.early + o.halvings)))) for o in c.octaves)


def padded(y, left, right, pad, pad_value):
    """The boundary extension of Stft's centered alignment (stft.ml:300-338) on the last axis."""
    n = y.shape[-1]
    q = np.arange(-left, n + right)
    if pad == "constant":
        out = np.full(y.shape[:-1] + (q.size,), pad_value, dtype=y.dtype)
        inside = (q >= 0) & (q < n)
        out[..., inside] = y[..., q[inside]]
        return out
    if pad == "edge":
        return y[..., np.clip(q, 0, n - 1)]
    if n == 1:
        return y[..., np.zeros_like(q)]
    period = 2 * (n - 1)
    m = np.mod(q, period)
    return y[..., np.where(m < n, m, period - m)]


def octave_spectrum(o, y, count, pad, pad_value):
    """``Stft.transform`` of the octave's rectangular centered analysis, first ``count`` frames: [...; n_fft / 2 + 1; count]."""
    half = o.n_fft // 2
    yp = padded(y, half, half, pad, pad_value)
    idx = (np.arange(count) * o.hop)[:, None] + np.arange(o.n_fft)[None, :]
    return np.moveaxis(np.fft.rfft(yp[..., idx], axis=-1), -1, -2)


def transform(c, x, decimate):
    """``Cqt.transform`` (cqt.ml:615-667) in complex128; ``decimate(y)`` is the exact 2:1 conversion of the last axis.
    The octave signals are float64 here whatever the decimator computes in."""
    x = np.asarray(x, dtype=np.float64)
    count = frames(c, x.shape[-1])
    lead = x.shape[:-1]
    if 0 in lead or count == 0:
        return np.zeros(lead + (c.n_bins, max(0, count)), dtype=np.complex128)
    y = x
    if c.early > 0:
        for _ in range(c.early):
            y = np.asarray(decimate(y), dtype=np.float64)
        factor = math.sqrt(float(1 << c.early))
        y = y * factor
        if not c.scale:
            y = y * factor
    out = np.zeros(lead + (c.n_bins, count), dtype=np.complex128)
    last = len(c.octaves) - 1
    for i, o in enumerate(c.octaves):
        d = octave_spectrum(o, y, count, c.pad, c.pad_value)
        out[..., o.first:o.first + o.count, :] = np.matmul(o.kernel, d)
        if i < last and o.hop % 2 == 0:
            y = np.asarray(decimate(y), dtype=np.float64) / math.sqrt(0.5)
    if c.divisors is not None:
        out = out / c.divisors[:, None]
    return out


def power_spectrum(c, x, decimate, power=2.0):   # cqt.ml:671-692
    m = np.abs(transform(c, x, decimate))
    return m * m if power == 2.0 else (m if power == 1.0 else m ** power)


def no_decimation(y):
    raise AssertionError("this plan must not decimate")


# ---- chroma.ml:332-385 ---------------------------------------------------------------------------------------------------

def round_half_even(x):
    below = math.floor(x)
    fraction = x - below
    if fraction > 0.5:
        return below + 1.0
    if fraction < 0.5:
        return below
    return below if math.fmod(below, 2.0) == 0.0 else below + 1.0


def cqt_projection(n_chroma, bins_per_octave, n_bins, fmin, op="cqt_projection"):
    if n_chroma < 1:
        raise ValueError("%s: cannot build %d chroma bands (n_chroma must be at least 1)" % (op, n_chroma))
    if bins_per_octave % n_chroma != 0:
        raise ValueError("%s: cannot fold %d bins per octave onto %d chroma bands (bins_per_octave must be an integer multiple "
                         "of n_chroma)" % (op, bins_per_octave, n_chroma))
    merge = bins_per_octave // n_chroma
    midi = (12.0 * (math.log2(fmin) - math.log2(440.0))) + 69.0
    midi = math.fmod(math.fmod(midi, 12.0) + 12.0, 12.0)
    shift = int(round_half_even(midi * (float(n_chroma) / 12.0)))
    w = np.zeros((n_chroma, n_bins))
    for ch in range(n_chroma):
        source = (((ch - shift) % n_chroma) + n_chroma) % n_chroma
        for k in range(n_bins):
            step = ((k % bins_per_octave) + (merge // 2)) % bins_per_octave
            if step // merge == source:
                w[ch, k] = 1.0
    return w


def normalise(raw, norm, tiny):   # chroma.ml:56-82
    if norm is None or norm == "none":
        return raw
    mag = np.abs(raw)
    if norm == "inf":
        lengths = np.max(mag, axis=-2, keepdims=True)
    elif norm == 1.0:
        lengths = np.sum(mag, axis=-2, keepdims=True)
    elif norm == 2.0:
        lengths = np.sqrt(np.sum(mag * mag, axis=-2, keepdims=True))
    else:
        lengths = np.sum(mag ** norm, axis=-2, keepdims=True) ** (1.0 / norm)
    return raw / np.where(lengths < tiny, 1.0, lengths)


def of_cqt(c, s, n_chroma=12, norm="inf", tiny=2.0 ** -126):
    w = cqt_projection(n_chroma, c.bins_per_octave, c.n_bins, c.fmin, "of_cqt")
    return normalise(np.matmul(w, np.asarray(s, dtype=np.float64)), norm, tiny)
