"""Plain-numpy float64 restatement of the reference's time-scale and pitch modification (soundml/lib/effects.ml), the
yardstick of the Effects tests.  A test helper, not part of the product: written from the module's documented semantics,
on the oracle's ``transform`` / ``invert``.

The vocoder's phases are a recurrence whose accumulator reaches 1e6 rad, so agreement with the reference at 1e-11 needs
the same float64 operations in the same order.  numpy's elementwise float64 ``+ - * /``, ``rint`` and ``hypot`` (``abs`` of a
complex) are those operations, the argument is libm's ``atan2`` (``polar``); every bracket below is the reference's.
"""
import json
import math
import os

import numpy as np
import pytest

from oracle import soundml_oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pvoc")
TWO_PI = 2.0 * math.pi
RATIO_CAP = 512
GOLDEN_SEED = 20250803          # pvoc_goldens.ml:65-69, 86-88
FLOAT64_ATOL = 1e-11            # pvoc_goldens.ml:44
PITCH_FRACTION = 4e-2           # pvoc_goldens.ml:63


def golden_cases(name):
    """The cases of the reference's vector file soundml/test/pvoc/vectors/<name>.json as pytest parameters, each
    {"name", "params", "shape", "values"}.  The four files are committed repacked, values untouched: cases.json holds every
    case's name, shape and parameters as one table row, <name>.npz its float64 values under the case's name."""
    with open(os.path.join(GOLDEN, "cases.json")) as fh:
        table = json.load(fh)[name]
    values = np.load(os.path.join(GOLDEN, name + ".npz"))
    columns = table["columns"][2:]
    return [pytest.param({"name": row[0], "shape": row[1], "params": dict(zip(columns, row[2:])), "values": values[row[0]]},
                         id=row[0]) for row in table["rows"]]


def golden_config(params):
    """pvoc_goldens.ml:71-76: librosa's zero padding, centred frames."""
    return O.stft_config(params["fft_size"], hop=params["hop"], pad="constant", pad_value=0.0)


def golden_signal(params):
    """pvoc_goldens.ml:78-88: one LCG stream over the whole shape, float64; float32 cases quantise it."""
    n, channels = params["n"], params["channels"]
    shape = (n,) if channels == 1 else (channels, n)
    return O.lcg_signal(int(np.prod(shape)), GOLDEN_SEED).reshape(shape).astype(params["dtype"])


def round_half_even(x):
    return float(np.rint(x))


def principal(x):
    """effects.ml:79: x reduced to the interval of width 2 pi centred at zero, ties to even."""
    return x - (TWO_PI * np.rint(x / TWO_PI))


def advance(fft_size, hop, bins):
    """effects.ml:83-86: the phase a bin centre advances over one hop; never reduced."""
    step = 1.0 / (float(fft_size) * (1.0 / TWO_PI))
    return float(hop) * (np.arange(bins, dtype=np.float64) * step)


_ATAN2 = np.frompyfunc(math.atan2, 2, 1)


def polar(z):
    """(magnitude, argument) of a complex array in float64.  The argument is libm's atan2 cell by cell, the function the
    reference calls: numpy's own ``angle`` runs a vectorised kernel that differs from it in the last bit of one cell in
    thirteen, which the recurrence below turns into whole ulps of a 1e5-rad accumulator."""
    z = np.asarray(z).astype(np.complex128)
    return np.abs(z), _ATAN2(z.imag, z.real).astype(np.float64)


def out_frames(frames, rate):
    """effects.ml:90-92."""
    return 0 if frames == 0 else int(math.ceil(float(frames) / rate))


def stretch_length(n, rate):
    """effects.ml:295."""
    return int(round_half_even(float(n) / rate))


def peaks_of(m):
    """effects.ml:146-160: the bins strictly above each of the up to four neighbours they have."""
    bins = m.shape[0]
    peak = np.ones(bins, dtype=bool)
    for d in (-2, -1, 1, 2):
        j = np.arange(bins) + d
        ok = (j >= 0) & (j < bins)
        above = np.ones(bins, dtype=bool)
        above[ok] = m[ok] > m[j[ok]]
        peak &= above
    return np.flatnonzero(peak)


def lock(phi, ang, peaks):
    """effects.ml:167-182: every bin of a peak's region takes the peak's phase plus its own analysis phase difference;
    regions split at (kp + kp_next + 1) / 2, the first starts at bin 0 and the last ends at the top."""
    bins = phi.shape[0]
    stops = (peaks[:-1] + peaks[1:] + 1) // 2
    owner = peaks[np.searchsorted(stops, np.arange(bins), side="right")]
    locked = phi[owner] + (ang - ang[owner])
    locked[peaks] = phi[peaks]
    return locked


def vocode(fft_size, hop, z, rate, locked=False, parts=None):
    """effects.ml:184-274: complex [...; bins; frames] -> complex128 [...; bins; count].  parts: ``polar(z)`` where the
    caller already has it (it does not depend on the rate or the phase mode)."""
    z = np.asarray(z).astype(np.complex128)
    bins, frames = z.shape[-2], z.shape[-1]
    lead = z.shape[:-2]
    count = out_frames(frames, rate)
    signals = int(np.prod(lead)) if lead else 1
    if signals == 0 or count == 0:
        return np.zeros(lead + (bins, count), dtype=np.complex128)
    magnitude, argument = polar(z) if parts is None else parts
    mag = np.zeros((signals, frames + 2, bins))                             # [signals; frames + 2; bins], two rows of silence
    ang = np.zeros((signals, frames + 2, bins))
    mag[:, :frames] = np.swapaxes(magnitude.reshape(signals, bins, frames), -1, -2)
    ang[:, :frames] = np.swapaxes(argument.reshape(signals, bins, frames), -1, -2)
    omega = advance(fft_size, hop, bins)
    amp = np.zeros((signals, count, bins))
    phases = np.zeros((signals, count, bins))
    phi = ang[:, 0].copy()
    for i in range(count):
        position = float(i) * rate
        i0 = int(position)
        alpha = position - float(i0)
        amp[:, i] = ((1.0 - alpha) * mag[:, i0]) + (alpha * mag[:, i0 + 1])
        if locked:
            for s in range(signals):
                peaks = peaks_of(mag[s, i0])
                if peaks.size:
                    phi[s] = lock(phi[s], ang[s, i0], peaks)
        phases[:, i] = phi
        if i + 1 < count:
            deviation = principal(ang[:, i0 + 1] - ang[:, i0] - omega)
            phi = phi + (omega + deviation)
    out = (amp * np.cos(phases)) + 1j * (amp * np.sin(phases))
    return np.swapaxes(out, -1, -2).reshape(lead + (bins, count))


def phase_vocoder(c, z, rate, locked=False):
    """effects.ml:285-289: in the dtype of z, one rounding."""
    z = np.asarray(z)
    return vocode(c.fft_size, c.hop, z, rate, locked).astype(z.dtype)


def time_stretch(c, x, rate, locked=False):
    """effects.ml:291-298: complex128 spectra between the three stages, the result in x's dtype."""
    x = np.asarray(x)
    length = stretch_length(x.shape[-1], rate)
    z = O.transform(c, x, np.complex128)
    return O.invert(c, vocode(c.fft_size, c.hop, z, rate, locked), length, x.dtype)


def resample_stage(proto, l, m, k, x):
    """One polyphase stage by its definition, evaluated sparsely: y[i] = sum_q x[q] proto[i M + K L - q L] over the at most
    2 K + 1 samples whose tap exists, ceil(n L / M) outputs, float64."""
    x = np.asarray(x, dtype=np.float64)
    proto = np.asarray(proto, dtype=np.float64)
    n = x.shape[-1]
    n_out = -(-n * l // m)
    if n_out == 0:
        return np.zeros(x.shape[:-1] + (0,))
    i = np.arange(n_out, dtype=np.int64)[:, None]
    q = (i * m + k * l) // l - np.arange(2 * k + 1, dtype=np.int64)[None, :]
    t = i * m + k * l - q * l
    ok = (t >= 0) & (t < proto.shape[0]) & (q >= 0) & (q < n)
    taps = np.where(ok, proto[np.clip(t, 0, proto.shape[0] - 1)], 0.0)         # [n_out; 2 K + 1]
    return np.einsum("...ij,ij->...i", x[..., np.clip(q, 0, n - 1)], taps)


def fix_length(n, y):
    """effects.ml:302-314."""
    have = y.shape[-1]
    if have >= n:
        return y[..., :n]
    return np.concatenate([y, np.zeros(y.shape[:-1] + (n - have,), dtype=y.dtype)], axis=-1)


def pitch_shift(c, x, ratio, resampler, locked=False):
    """effects.ml:324-334 with this library's single-stage resampler: ``resampler`` is the ``Resample.Config`` built for
    num -> den (its prototype, rate and latency need no device)."""
    x = np.asarray(x)
    num, den = ratio
    stretched = time_stretch(c, x, float(den) / float(num), locked)
    l, m = resampler.rate
    if (l, m) != (1, 1):
        stretched = resample_stage(resampler.prototype(), l, m, resampler.latency, stretched).astype(x.dtype)
    return fix_length(x.shape[-1], stretched)


def semitones(n, bins_per_octave=12):
    """effects.ml:345-386: denominators 1..512, the error compared in log2, the first best kept, reduced by the gcd."""
    if bins_per_octave < 1:
        raise ValueError("semitones: cannot divide the octave into %d steps (bins_per_octave must be at least 1)" % bins_per_octave)
    n = float(n)
    if not math.isfinite(n):
        raise ValueError("semitones: cannot shift by %s steps (the step count must be finite)"
                         % ("nan" if math.isnan(n) else ("inf" if n > 0 else "-inf")))
    target = math.pow(2.0, n / float(bins_per_octave))
    best = None
    for den in range(1, RATIO_CAP + 1):
        num = int(round_half_even(target * float(den)))
        if 1 <= num <= RATIO_CAP:
            error = abs(math.log2(float(num) / float(den)) - math.log2(target))
            if best is None or not best[0] <= error:
                best = (error, num, den)
    if best is None:
        raise ValueError("semitones: cannot represent a frequency ratio of %g within %d (the step count is too far from unity)"
                         % (target, RATIO_CAP))
    d = math.gcd(best[1], best[2])
    return best[1] // d, best[2] // d
