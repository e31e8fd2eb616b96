"""The numpy restatement of Mel.invert and mfcc_to_mel (tests/inversion_restatement.py) against what does not depend on it: the
structure of the oracle's filterbanks, the exact minimum 0 of consistent targets, the oracle's own mfcc.  The residuals it
reaches after 200 rounds are recorded in tests/golden/inversion/residuals.json; the GPU suite gates the device on them."""
import numpy as np
import pytest

from conftest import load_golden
from oracle import soundml_oracle as O

import inversion_restatement as R

RECORDED = load_golden("inversion", "residuals")


@pytest.mark.parametrize("name", sorted(R.BANKS))
def test_bank_structure(name):
    """what the solver relies on: a bin lies in at most two filters, and they are neighbours, so W W^T is tridiagonal; the
    Gershgorin bound is an upper bound of the largest eigenvalue and within 10 % of it"""
    w = R.bank_weights(name)
    touched = (w != 0.0).sum(axis=0)
    assert touched.max() <= 2
    for k in np.flatnonzero(touched == 2):
        j = np.flatnonzero(w[:, k])
        assert j[1] == j[0] + 1
    g = w @ w.T
    off = np.abs(g - np.diag(np.diag(g)) - np.diag(np.diag(g, 1), 1) - np.diag(np.diag(g, -1), -1))
    assert off.max() == 0.0
    top = float(np.linalg.eigvalsh(g)[-1])
    assert top <= R.lipschitz(w) <= 1.10 * top


@pytest.fixture(scope="module")
def solved():
    out = {}
    for name in R.BANKS:
        w = R.bank_weights(name)
        s_true = R.synthetic_spectra(w.shape[1], R.RESIDUAL_FRAMES)
        m = w @ s_true
        out[name] = (w, m, R.mel_invert(w, m, 200, np.float64))
    return out


@pytest.mark.parametrize("name", sorted(R.BANKS))
def test_recorded_residuals(name, solved):
    """consistent targets m = W s: the minimum is 0, the iterate is non-negative, untouched bins stay 0, and the residual
    after 200 rounds is the recorded one"""
    w, m, s = solved[name]
    assert s.dtype == np.float64 and (s >= 0.0).all()
    assert not s[(w != 0.0).sum(axis=0) == 0].any()
    res = R.relative_residual(w, s, m)
    rec = RECORDED[name]
    assert rec["frames"] == R.RESIDUAL_FRAMES
    np.testing.assert_allclose(float(res.max()), rec["residual_200"], rtol=1e-3)     # (the targets come from a BLAS product)
    assert res.max() < 0.01


@pytest.mark.parametrize("name", ["fft64_mel8", "fft400_mel80", "fft2048_mel128"])
def test_float32_follows_float64(name, solved):
    """the same rounds in float32: the recorded distance from the float64 iterate, relative to the frame's largest value (the
    GPU suite allows the device four times it), and a residual within a factor 2 + 1e-5 of the float64 one"""
    w, m, s64 = solved[name]
    s32 = R.mel_invert(w, m[:, :64], 200, np.float32)
    assert s32.dtype == np.float32
    dist = np.abs(s32.astype(np.float64) - s64[:, :64]).max(axis=0) / s64[:, :64].max(axis=0)
    assert float(dist.max()) <= RECORDED[name]["float32_distance_200"] * 1.25
    res32 = R.relative_residual(w, s32, m[:, :64].astype(np.float32))
    assert (res32 <= 2.0 * RECORDED[name]["residual_200"] + 1e-5).all()


def test_zero_rounds_and_snapshots():
    w = R.bank_weights("fft64_mel8")
    m = w @ R.synthetic_spectra(33, 5)
    s, snap = R.mel_invert(w, m, 7, np.float64, snapshots=(0, 1, 7))
    assert not snap[0].any()
    assert np.array_equal(snap[7], s) and np.array_equal(snap[1], R.mel_invert(w, m, 1, np.float64))
    assert not R.mel_invert(w, m, 0, np.float32).any()


@pytest.mark.parametrize("lifter", [None, 22.0])
def test_mfcc_to_mel_undoes_the_oracles_mfcc(lifter):
    """float64 against the float64 oracle, n_mfcc = n_mels: wherever the 80 dB clamp (and the amin floor) did not act the mel
    spectrogram comes back; a DCT pair and a log / exp pair in double"""
    sc, mc = O.stft_config(256, hop=64), O.mel_config(20, 8000, 256)
    x = O.harmonic_signal(4000, 8000).astype(np.float64).reshape(1, -1)
    mel = O.mel_spectrogram(sc, mc, x)
    c = O.mfcc(sc, mc, x, n_mfcc=20, lifter=lifter)
    got = R.mfcc_to_mel(c, 20, lifter)
    assert got.shape == mel.shape
    free = mel > max(1e-10, float(mel.max()) * 10.0 ** -8.0) * (1.0 + 1e-9)
    assert free.sum() > mel.size // 4
    np.testing.assert_allclose(got[free], mel[free], rtol=1e-9, atol=0)


def test_mfcc_to_mel_pads_the_cepstral_axis():
    """fewer coefficients than bands: the missing rows count as zeros"""
    rng = np.random.default_rng(5)
    c = rng.normal(size=(2, 6, 9))
    padded = np.concatenate([c, np.zeros((2, 14, 9))], axis=1)
    np.testing.assert_allclose(R.mfcc_to_mel(c, 20, reference=2.5), R.mfcc_to_mel(padded, 20, reference=2.5), rtol=1e-13)
