"""numpy restatement of ``Mel.invert`` (DESIGN.md "Mel inversion") in float64 and float32, and of ``mfcc_to_mel``.

The solver's order is the stated one: per mel row a chain of fused multiply-adds over the row's band in ascending bins from
-m_j, per bin the product of its first filter's weight and residual with the second fused onto it, the projected step, the
momentum step.  numpy has no fused multiply-add: float32 takes the product and the sum in float64 and rounds once (exact but
for a double rounding), float64 takes a * b + c.  All frames advance together; nothing couples them.
"""
import math

import numpy as np

from oracle import soundml_oracle as O

# name -> (n_mels, sample_rate, fft_size, scale, norm): the five filterbanks the solver's facts were checked on
BANKS = {
    "fft64_mel8": (8, 8000, 64, "slaney", "slaney"),
    "fft32_mel5_htk": (5, 8000, 32, "htk", "none"),
    "fft512_mel40_htk": (40, 16000, 512, "htk", "none"),
    "fft2048_mel128": (128, 22050, 2048, "slaney", "slaney"),
    "fft400_mel80": (80, 16000, 400, "slaney", "slaney"),
}
RESIDUAL_FRAMES = 280    # the recorded residual is the largest over this many synthetic frames


def bank_weights(name):
    n_mels, sr, fft, scale, norm = BANKS[name]
    return O.mel_config(n_mels, sr, fft, scale=scale, norm=norm).weights


def synthetic_spectra(bins, count, first=0):
    """[bins; count] non-negative float64 spectra without a random generator: a floor and three moving bumps per frame."""
    k = np.arange(bins, dtype=np.float64)[:, None]
    t = np.arange(first, first + count, dtype=np.float64)[None, :] + 1.0
    s = np.full((bins, count), 0.01)
    for i, (phi, width, amp) in enumerate(((0.6180339887, 0.02, 1.0), (0.4142135623, 0.05, 0.5), (0.7320508075, 0.11, 0.25))):
        centre = bins * np.mod(t * phi + 0.1 * i, 1.0)
        w = max(1.0, width * bins)
        s = s + amp * (1.0 + 0.5 * np.sin(t * (i + 1))) * np.exp(-0.5 * ((k - centre) / w) ** 2)
    return s


def lipschitz(w):
    """Gershgorin: the largest absolute row sum of W W^T, float64."""
    return float(np.max(np.sum(np.abs(w @ w.T), axis=1)))


def betas(n_iter):
    out, t = [], 1.0
    for _ in range(n_iter):
        nxt = (1.0 + math.sqrt(1.0 + 4.0 * t * t)) / 2.0
        out.append((t - 1.0) / nxt)
        t = nxt
    return out


def _fma(dtype):
    if dtype == np.float32:
        return lambda a, b, c: (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)
    return lambda a, b, c: a * b + c


def mel_invert(w, m, n_iter=200, dtype=np.float64, snapshots=()):
    """m [n_mels; frames] -> s [bins; frames] in `dtype`; with snapshots = (k1, k2, ...) a dict {k: s after k rounds} as well."""
    dtype = np.dtype(dtype).type
    fma = _fma(dtype)
    n_mels, bins = w.shape
    frames = m.shape[1]
    wt = w.astype(dtype)
    m = m.astype(dtype)
    nz = w != 0.0
    lo = np.array([np.flatnonzero(r)[0] if r.any() else 0 for r in nz])
    ln = np.array([np.flatnonzero(r)[-1] + 1 - np.flatnonzero(r)[0] if r.any() else 0 for r in nz])
    # per bin its at most two filters, ascending
    j0 = np.full(bins, -1)
    j1 = np.full(bins, -1)
    for k in range(bins):
        js = np.flatnonzero(nz[:, k])
        assert len(js) <= 2, "bin %d lies in %d filters" % (k, len(js))
        if len(js) > 0:
            j0[k] = js[0]
        if len(js) > 1:
            j1[k] = js[1]
    live, two = j0 >= 0, j1 >= 0
    w0 = np.where(live, wt[np.maximum(j0, 0), np.arange(bins)], 0).astype(dtype)[:, None]
    w1 = np.where(two, wt[np.maximum(j1, 0), np.arange(bins)], 0).astype(dtype)[:, None]
    big = lipschitz(w)
    eta = dtype(1.0 / big if big > 0.0 else 0.0)
    s = np.zeros((bins, frames), dtype=dtype)
    y = np.zeros((bins, frames), dtype=dtype)
    taken = {}
    if 0 in snapshots:
        taken[0] = s.copy()
    for it, beta in enumerate(betas(n_iter)):
        beta = dtype(beta)
        r = -m
        for q in range(int(ln.max()) if n_mels else 0):
            rows = np.flatnonzero(ln > q)
            r[rows] = fma(wt[rows, lo[rows] + q][:, None], y[lo[rows] + q], r[rows])
        g = w0 * r[np.maximum(j0, 0)]
        g = np.where(two[:, None], fma(w1, r[np.maximum(j1, 0)], g), g)
        sn = np.maximum(fma(np.broadcast_to(-eta, g.shape), g, y), dtype(0))
        sn = np.where(live[:, None], sn, dtype(0)).astype(dtype)
        y = fma(np.broadcast_to(beta, sn.shape), sn - s, sn)
        s = sn
        if it + 1 in snapshots:
            taken[it + 1] = s.copy()
    return (s, taken) if snapshots else s


def relative_residual(w, s, m):
    """|W s - m| / |m| per frame, float64."""
    s, m = s.astype(np.float64), m.astype(np.float64)
    return np.linalg.norm(w @ s - m, axis=0) / np.linalg.norm(m, axis=0)


def lifter_weights(n_mfcc, lifter):
    if lifter is None or lifter <= 0.0:
        return np.ones(n_mfcc)
    return 1.0 + lifter / 2.0 * np.sin(np.pi * (np.arange(n_mfcc, dtype=np.float64) + 1.0) / lifter)


def mfcc_to_mel(c, n_mels, lifter=None, reference=1.0):
    """[...; n_mfcc; frames] -> [...; n_mels; frames], float64: un-lifter, orthonormal scale, transposed DCT-II rows over the
    coefficients that exist, reference * 10 ** (db / 10)."""
    c = np.asarray(c, dtype=np.float64)
    n_mfcc = c.shape[-2]
    k = np.arange(n_mfcc, dtype=np.float64)[:, None]
    mm = np.arange(n_mels, dtype=np.float64)[None, :]
    raw = 2.0 * np.cos(np.pi * k * (2.0 * mm + 1.0) / (2.0 * n_mels))
    scales = np.where(np.arange(n_mfcc) == 0, 1.0 / math.sqrt(4.0 * n_mels), 1.0 / math.sqrt(2.0 * n_mels))
    v = c / lifter_weights(n_mfcc, lifter)[:, None] * scales[:, None]
    db = np.einsum("km,...kt->...mt", raw, v)
    return reference * 10.0 ** (db / 10.0)
