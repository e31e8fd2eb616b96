"""Plain-numpy restatement of the reference's harmonic/percussive separation (soundml/lib/hpss.ml), the yardstick of
the Hpss tests.  A test helper, not part of the product: written from the module's documented semantics.

A median SELECTS, so the spectrogram-domain faces are reproducible bit for bit in the dtype of the input: every step
below runs in that dtype (numpy's float32 division, multiplication and comparison are correctly rounded).
"""
import json
import os

import numpy as np
import pytest

from oracle import soundml_oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hpss")


def golden_cases(name):
    """The cases of the reference's vector file soundml/test/hpss/vectors/<name>.json as pytest parameters, each
    {"name", "params", "shape", "values"} as conftest.load_golden gives them.  The four files are committed repacked, values
    untouched: cases.json holds every case's name, shape and parameters as one table row, values.npz its values under
    "<name>/<case>" in the narrowest of uint8 / float32 / float64 that holds every value of the case exactly."""
    with open(os.path.join(GOLDEN, "cases.json")) as fh:
        table = json.load(fh)[name]
    values = np.load(os.path.join(GOLDEN, "values.npz"))
    columns = table["columns"][2:]
    return [pytest.param({"name": row[0], "shape": row[1], "params": dict(zip(columns, row[2:])),
                          "values": values["%s/%s" % (name, row[0])].astype(np.float64)}, id=row[0])
            for row in table["rows"]]


def refl(i, n):
    """Half-sample-symmetric reflection into [0, n), period 2 n: -1 -> 0, n -> n - 1; total (hpss.ml:69-75)."""
    j = np.mod(i, 2 * n)
    return np.where(j < n, j, 2 * n - 1 - j)


def running_median(s, k, axis):
    """Rank k // 2 of the ascending window [i - k // 2, i + k - 1 - k // 2] along ``axis`` (hpss.ml:43-50)."""
    s = np.asarray(s)
    n = s.shape[axis]
    if s.size == 0:
        return s.copy()
    idx = refl(np.arange(n)[:, None] - k // 2 + np.arange(k)[None, :], n)   # [n; k]
    moved = np.ascontiguousarray(np.moveaxis(s, axis, -1))
    out = np.empty(moved.shape, moved.dtype)
    flat_in, flat_out = moved.reshape(-1, n), out.reshape(-1, n)
    step = max(1, (1 << 24) // max(1, n * k))
    for lo in range(0, flat_in.shape[0], step):
        flat_out[lo:lo + step] = np.sort(flat_in[lo:lo + step][:, idx], axis=-1)[..., k // 2]
    return np.moveaxis(out, -1, axis)


def medians(s, kernel_size):
    k_h, k_p = kernel_size
    return running_median(s, k_h, -1), running_median(s, k_p, -2)


def powered(x, p):
    if p == 1.0:
        return x
    if p == 2.0:
        return x * x
    return np.power(x, x.dtype.type(p))


def softmask(x, r, power, split_zeros):
    """hpss.ml:325-338, in the dtype of x."""
    dt = x.dtype
    if not np.isfinite(power):
        return (x > r).astype(dt)
    z = np.maximum(x, r)
    bad = z < np.finfo(dt).tiny
    z = np.where(bad, dt.type(1), z)
    with np.errstate(invalid="ignore", divide="ignore"):
        m = powered(x / z, power)
        q = powered(r / z, power)
        share = m / (m + q)
    return np.where(bad, dt.type(0.5 if split_zeros else 0.0), share).astype(dt)


def hpss_masks(s, kernel_size=(31, 31), power=2.0, margin=(1.0, 1.0)):
    s = np.asarray(s)
    dt = s.dtype
    harm, perc = medians(s, kernel_size)
    m_h, m_p = dt.type(margin[0]), dt.type(margin[1])
    split = margin[0] == 1.0 and margin[1] == 1.0
    return softmask(harm, perc * m_h, power, split), softmask(perc, harm * m_p, power, split)


def hpss_of_spectrogram(s, kernel_size=(31, 31), power=2.0, margin=(1.0, 1.0)):
    s = np.asarray(s)
    mask_h, mask_p = hpss_masks(s, kernel_size, power, margin)
    return s * mask_h, s * mask_p


def of_stft_parts(z, kernel_size=(31, 31), power=2.0, margin=(1.0, 1.0)):
    """(mag, harm, perc, z_h, z_p) of hpss.ml:436-459 in the component width of z."""
    z = np.asarray(z)
    rdt = np.float32 if z.dtype == np.complex64 else np.float64
    mag = np.abs(z).astype(rdt)
    one_at_zero = (mag == 0).astype(rdt)
    denominator = mag + one_at_zero
    phase_re = z.real.astype(rdt) / denominator + one_at_zero
    phase_im = z.imag.astype(rdt) / denominator
    harm, perc = medians(mag, kernel_size)
    mask_h, mask_p = hpss_masks(mag, kernel_size, power, margin)

    def apply(mask):
        t = mag * mask
        out = np.empty(z.shape, z.dtype)
        out.real = t * phase_re
        out.imag = t * phase_im
        return out
    return mag, harm, perc, apply(mask_h), apply(mask_p)


def hpss_of_stft(z, kernel_size=(31, 31), power=2.0, margin=(1.0, 1.0)):
    return of_stft_parts(z, kernel_size, power, margin)[3:]


def hpss(c, x, kernel_size=(31, 31), power=2.0, margin=(1.0, 1.0)):
    """hpss.ml:477-492 on the oracle's transform / invert (float64 interior): x [...; n] -> (y_h, y_p) in x's dtype."""
    x = np.asarray(x)
    cdt = np.complex128 if x.dtype == np.float64 else np.complex64
    z_h, z_p = hpss_of_stft(O.transform(c, x, cdt), kernel_size, power, margin)
    n = x.shape[-1]
    return O.invert(c, z_h, n, x.dtype), O.invert(c, z_p, n, x.dtype)


# ---- the goldens' inputs (soundml/test/hpss/hpss_goldens.ml:38-75) ----------------------------------------------------
def golden_spectrogram(params):
    """One folded LCG draw per cell, a constant ridge on every seventh bin and a constant column on every fifth frame,
    in that order, the top ``silent_bins`` bins zero; the batched cell stacks the plane with its half.  float64."""
    bins, frames = params["bins"], params["frames"]
    v = np.abs(O.lcg_signal(bins * frames, params["seed"])).reshape(bins, frames)
    b, t = np.arange(bins)[:, None], np.arange(frames)[None, :]
    v = v + np.where(b % 7 == 3, 3.0, 0.0)
    v = v + np.where(t % 5 == 2, 2.0, 0.0)
    v = np.where(b >= bins - params["silent_bins"], 0.0, v)
    if params["planes"] == 1:
        return v
    return np.stack([v, v * 0.5])


def golden_arguments(params):
    return dict(kernel_size=(params["kernel_h"], params["kernel_p"]), power=float(params["power"]),
                margin=(params["margin_h"], params["margin_p"]))


def component(params, pair):
    return pair[0] if params["component"] == "harmonic" else pair[1]
