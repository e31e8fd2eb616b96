"""The numpy restatement of Pitch (tests/pitch_restatement.py) is itself checked here, without a device: against an independent
direct form of the difference function, on harmonic tones of known pitch, on silence and noise, and against another summation
order (so that the bit-for-bit gates of test_gpu_pitch.py can fail)."""
import numpy as np
import pytest

import pitch_restatement as R

SR, FL, HOP, FMIN, FMAX = 22050, 2048, 512, 65.0, 2093.0
TONES = [82.41, 110.0, 220.0, 440.0, 523.25, 987.77]


def direct_difference(f, pmax):
    """sum_{j < W} (x_j - x_{j + tau})^2 in float64, np.sum's own order"""
    W = f.shape[-1] // 2
    return np.stack([np.sum(np.square(f[..., :W] - f[..., tau:tau + W]), axis=-1) for tau in range(pmax + 1)], axis=-1)


@pytest.mark.parametrize("frame_length,hop,n,sr,fmin,fmax", [(2048, 512, 5000, 22050, 65, 2093), (200, 64, 900, 8000, 100, 1000),
                                                             (33, 7, 90, 8000, 600, 3000)])
def test_energy_form_against_the_direct_form(frame_length, hop, n, sr, fmin, fmax):
    """|d - d_direct| <= 4 W 2^-53 (e(0) + e(tau)): three sequential sums of W terms behind d (r, and the two energies) plus the
    direct form's own.  (e is a difference of two prefixes here, each a chain of at most tau + W <= 2 W terms over samples whose
    squares e(0) + e(tau) bounds; the bound is the issue's, the figures printed are far inside it.)"""
    pmax = R.lag_range(sr, fmin, fmax, frame_length)[1]
    W = frame_length // 2
    for x in (R.decades(n, 3, n, np.float32), np.random.default_rng(n).uniform(-1, 1, size=(2, n)).astype(np.float32),
              R.decades(n + 1, 2, n, np.float64)):
        f = R.padded_frames(x, frame_length, hop)
        d, e = R.difference(f, hop, pmax)
        direct = direct_difference(f, pmax)
        bound = 4.0 * W * 2.0 ** -53 * (e[..., :1] + e)
        err = np.abs(d - direct)[..., 1:]
        worst = float(np.max(err / np.maximum(bound[..., 1:], np.finfo(np.float64).tiny)))
        print("%s %s: worst |d - d_direct| / bound = %.3g" % ((frame_length, hop, n), x.dtype, worst))
        assert np.all(err <= bound[..., 1:])


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_harmonic_tones(dtype):
    """interior frames within 3e-3 relative of the true f0, aperiodicity below 0.1"""
    worst_err, worst_ap = 0.0, 0.0
    for tone in TONES:
        x = R.harmonic_tone(tone, 8192, SR, dtype)
        f0, ap = R.yin(x, FMIN, FMAX, SR, FL, HOP)
        assert f0.shape == ap.shape == (1, R.frames(8192, FL, HOP)) and f0.dtype == dtype
        f0, ap = f0[0, 3:-3].astype(np.float64), ap[0, 3:-3].astype(np.float64)
        assert f0.size >= 8
        err = float(np.max(np.abs(f0 - tone) / tone))
        print("%s %.2f Hz: worst relative error %.3g, worst aperiodicity %.3g" % (np.dtype(dtype).name, tone, err, float(ap.max())))
        worst_err, worst_ap = max(worst_err, err), max(worst_ap, float(ap.max()))
        assert err <= 3e-3 and np.all(ap < 0.1), tone
    print("worst case: %.3g relative, aperiodicity %.3g" % (worst_err, worst_ap))


def test_silence_and_noise():
    pmin, pmax = R.lag_range(SR, FMIN, FMAX, FL)
    assert (pmin, pmax) == (10, 340)
    f0, ap = R.yin(np.zeros(8192, np.float32), FMIN, FMAX, SR)
    assert np.all(f0 == np.float32(SR / pmin)) and np.all(ap == 1.0)
    d = R.yin_difference(np.zeros((2, 3000)), FMIN, FMAX, SR)
    assert d.shape == (2, pmax + 1, R.frames(3000, FL, HOP)) and np.all(d == 1.0)
    x = np.random.default_rng(20260812).standard_normal(8192).astype(np.float32)
    f0, ap = R.yin(x, FMIN, FMAX, SR)
    print("white noise: least aperiodicity %.3g" % float(ap.min()))
    assert np.all(ap >= 0.1) and np.all(np.isfinite(f0))


def test_non_finite_samples_poison_the_frames_that_read_them():
    """a frame reads its first W + pmax samples (the lags end at pmax <= frame_length - W - 1): those frames give NaN, and no other"""
    fl, hop, n, sr, fmin, fmax = 64, 16, 300, 8000, 300.0, 2000.0
    span = R.used_span(fl, sr, fmin, fmax)
    assert span == 32 + 27
    x = R.signals(5, n, np.float32)
    clean = R.yin(x, fmin, fmax, sr, fl, hop)
    for bad in (np.nan, np.inf, -np.inf):
        y = x.copy()
        y[1, 150] = bad
        f0, ap = R.yin(y, fmin, fmax, sr, fl, hop)
        start = np.arange(f0.shape[-1]) * hop - fl // 2
        hit = (start <= 150) & (150 < start + span)
        assert hit.sum() == 4
        assert np.all(np.isnan(f0[1, 0, hit])) and np.all(np.isnan(ap[1, 0, hit]))
        keep = np.ones(f0.shape, bool)
        keep[1, 0, hit] = False
        assert np.array_equal(f0[keep], clean[0][keep]) and np.array_equal(ap[keep], clean[1][keep])


def test_another_summation_order_gives_other_bits():
    """noise scaled over 12 decades: r as one chain over all of j < W (no blocks), and with the blocks' chains descending"""
    fl, hop, n, sr, fmin, fmax = 256, 64, 1500, 8000, 100.0, 1000.0
    pmax = R.lag_range(sr, fmin, fmax, fl)[1]
    f = R.padded_frames(R.decades(7, 3, n, np.float32), fl, hop)
    ours = R.correlation(f, hop, pmax)
    one_chain = R.correlation(f, fl, pmax)
    descending = None
    for b0 in range(0, fl // 2, hop):
        acc = np.zeros(ours.shape)
        for j in reversed(range(b0, b0 + hop)):
            acc = acc + f[..., j:j + 1] * f[..., j:j + pmax + 1]
        descending = acc if descending is None else descending + acc
    for other in (one_chain, descending):
        assert np.allclose(other, ours, rtol=1e-9, atol=1e-9 * np.abs(ours).max())
        differ = np.mean(other != ours)
        print("another order: %.0f%% of the correlations differ in bits" % (100 * differ))
        assert differ > 0.05
    # and the difference reaches the outputs: d' in float32
    dn = R.yin_difference(R.decades(7, 3, n, np.float32), fmin, fmax, sr, fl, hop)
    assert dn.dtype == np.float32 and np.isfinite(dn).all()
