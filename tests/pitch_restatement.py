"""numpy restatement of Pitch (YIN; include/soundml_amd.h words the definition), no GPU.  Every add is explicit, nothing is left to
np.sum's pairwise tree: the one summation order of DESIGN.md 4.8f.

  r(tau)   j < W = frame_length // 2 in consecutive blocks of min(hop, W) from the frame's start; a block's partial is one ascending
           chain over j that starts from 0.0; the frame's r is the first block's partial, the others added in ascending order
  P(i)     the squares of the frame's samples in one ascending chain from its first sample, P(0) = 0;  e(tau) = P(tau + W) - P(tau)
  d, c, d' as written: d = max(0, (e(0) + e(tau)) - 2 r(tau)), c ascending, d' = (d tau) / c, 1 where c = 0

Float32 samples' products are exact in float64, so the kernel's fma and the multiply-then-add here give the same bits; float64
samples round the product, then the sum, in both.  This file is the yardstick of tests/test_gpu_pitch.py."""
import math

import numpy as np

import energy_restatement as E

frames = E.frames
decades = E.decades


def lag_range(sample_rate, fmin, fmax, frame_length):
    return int(math.floor(sample_rate / fmax)), int(min(math.ceil(sample_rate / fmin), frame_length - frame_length // 2 - 1))


def padded_frames(x, frame_length, hop):
    """[...; n] -> float64 [...; count; frame_length], zero borders"""
    return E.padded_frames(x, frame_length, hop, "constant")


def correlation(f, hop, pmax):
    """float64 frames [...; count; frame_length] -> r [...; count; pmax + 1]"""
    W = f.shape[-1] // 2
    blk, lags = min(hop, W), pmax + 1
    total = None
    with np.errstate(invalid="ignore"):
        for b0 in range(0, W, blk):
            acc = np.zeros(f.shape[:-1] + (lags,), np.float64)
            for j in range(b0, min(b0 + blk, W)):
                acc = acc + f[..., j:j + 1] * f[..., j:j + lags]
            total = acc if total is None else total + acc
    return total


def energies(f, pmax):
    """e [...; count; pmax + 1] from the running prefix of squares"""
    W = f.shape[-1] // 2
    prefix = np.zeros(f.shape[:-1] + (W + pmax + 1,), np.float64)
    for i in range(W + pmax):
        prefix[..., i + 1] = prefix[..., i] + f[..., i] * f[..., i]
    with np.errstate(invalid="ignore"):
        return prefix[..., W:W + pmax + 1] - prefix[..., :pmax + 1]


def difference(f, hop, pmax):
    """d [...; count; pmax + 1] (d(0) is not defined: 0 here)"""
    r, e = correlation(f, hop, pmax), energies(f, pmax)
    with np.errstate(invalid="ignore"):
        t = (e[..., :1] + e) - 2.0 * r
        d = np.where(t < 0.0, 0.0, t)            # a NaN stays one
    d[..., 0] = 0.0
    return d, e


def normalised(f, hop, pmax):
    """d' [...; count; pmax + 1], e(0) and c(pmax) [...; count]"""
    d, e = difference(f, hop, pmax)
    dn = np.ones_like(d)
    c = np.zeros(d.shape[:-1], np.float64)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for tau in range(1, pmax + 1):
            c = c + d[..., tau]
            dn[..., tau] = np.where(c == 0.0, 1.0, (d[..., tau] * float(tau)) / c)
    return dn, e[..., 0], c


def choose(dn, pmin, pmax, threshold):
    """one frame: the lag and the parabolic shift"""
    chosen = -1
    for tau in range(pmin, pmax + 1):
        if dn[tau] < threshold and dn[tau] <= dn[tau - 1] and (tau == pmax or dn[tau] < dn[tau + 1]):
            chosen = tau
            break
    if chosen < 0:
        chosen, least = pmin, dn[pmin]
        for tau in range(pmin + 1, pmax + 1):
            if dn[tau] < least:
                chosen, least = tau, dn[tau]
    shift = 0.0
    if chosen - 1 >= 1 and chosen + 1 <= pmax:
        a, b, c = dn[chosen - 1], dn[chosen], dn[chosen + 1]
        den = (a - 2.0 * b) + c
        if den > 0.0:
            s = (0.5 * (a - c)) / den
            if abs(s) <= 1.0:
                shift = s
    return chosen, shift


def yin_of_frames(f, hop, sample_rate, fmin, fmax, threshold, dtype):
    """float64 frames [...; count; frame_length] -> f0, aperiodicity [...; 1; count] in `dtype`"""
    pmin, pmax = lag_range(sample_rate, fmin, fmax, f.shape[-1])
    dn, e0, c = normalised(f, hop, pmax)
    flat = dn.reshape(-1, pmax + 1)
    f0, ap = np.empty(flat.shape[0], np.float64), np.empty(flat.shape[0], np.float64)
    sound = (np.isfinite(e0) & np.isfinite(c)).reshape(-1)
    for i in range(flat.shape[0]):
        tau, shift = choose(flat[i], pmin, pmax, threshold)
        f0[i], ap[i] = float(sample_rate) / (float(tau) + shift), flat[i, tau]
        if not sound[i]:
            f0[i] = ap[i] = np.nan
    shape = dn.shape[:-2] + (1, dn.shape[-2])
    return f0.reshape(shape).astype(dtype), ap.reshape(shape).astype(dtype)


def yin(x, fmin, fmax, sample_rate=22050, frame_length=2048, hop=None, threshold=0.1):
    hop = frame_length // 4 if hop is None else hop
    return yin_of_frames(padded_frames(x, frame_length, hop), hop, sample_rate, fmin, fmax, threshold, np.asarray(x).dtype)


def yin_difference(x, fmin, fmax, sample_rate=22050, frame_length=2048, hop=None):
    """[...; n] -> d' [...; pmax + 1; count] in the dtype of x"""
    hop = frame_length // 4 if hop is None else hop
    pmax = lag_range(sample_rate, fmin, fmax, frame_length)[1]
    dn = normalised(padded_frames(x, frame_length, hop), hop, pmax)[0]
    return np.ascontiguousarray(np.swapaxes(dn, -1, -2)).astype(np.asarray(x).dtype)


def used_span(frame_length, sample_rate, fmin, fmax):
    """the samples of a frame the definition reads: W + pmax of them from its start"""
    return frame_length // 2 + lag_range(sample_rate, fmin, fmax, frame_length)[1]


def harmonic_tone(f0, n=8192, sample_rate=22050, dtype=np.float64):
    t = np.arange(n) / float(sample_rate)
    return (np.sin(2 * np.pi * f0 * t) + 0.5 * np.sin(2 * np.pi * 2 * f0 * t) + 0.25 * np.sin(2 * np.pi * 3 * f0 * t)).astype(dtype)


def signals(seed, n, dtype):
    """3 clips of decade-scaled noise and one tone of 50.8 samples' period: [4; n]"""
    tone = harmonic_tone(0.0197, n, 1, np.float64)
    return np.concatenate([decades(seed, 3, n, np.float64), tone[None]], axis=0).astype(dtype)
