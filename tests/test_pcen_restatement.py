"""The numpy restatement of Pcen against scipy's lfilter (the smoother as librosa runs it) and against a direct transcription of
librosa.pcen's expressions, on the inputs and parameter sets of the device tests.  No GPU."""
import numpy as np
import pytest
import scipy.signal

from conftest import check_close

import pcen_restatement as R

CASES = [(name, scale) for name in R.SETS for scale in R.SCALES]
IDS = ["%s-scale%g" % c for c in CASES]


def librosa_pcen(S, sr=22050, hop_length=512, gain=0.98, bias=2, power=0.5, time_constant=0.4, eps=1e-6, b=None):
    """librosa.pcen (0.11, max_size=1, axis=-1) line for line; S is already scaled"""
    if b is None:
        t_frames = time_constant * sr / float(hop_length)
        b = (np.sqrt(1 + 4 * t_frames ** 2) - 1) / (2 * t_frames ** 2)
    ref = S
    zi = np.array([1 - b])                               # scipy.signal.lfilter_zi([b], [1, b - 1])
    assert np.allclose(zi, scipy.signal.lfilter_zi([b], [1, b - 1]), rtol=1e-13, atol=0)
    S_smooth, _ = scipy.signal.lfilter([b], [1, b - 1], ref, zi=zi * ref[..., 0:1], axis=-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        smooth = np.exp(-gain * (np.log(eps) + np.log1p(S_smooth / eps)))
        if power == 0:
            S_out = np.log1p(S * smooth / bias)
        elif bias == 0:
            S_out = np.exp(power * (np.log(S) + np.log(smooth)))
        else:
            S_out = (bias ** power) * np.expm1(power * np.log1p(S * smooth / bias))
    return S_out, S_smooth


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_the_restatement_is_librosa(case):
    name, scale = case
    kw = dict(R.SETS[name], scale=scale)
    worst = 0.0
    for shape in R.SHAPES:
        S = R.inputs(7, *shape)
        P, M, zf = R.pcen(S, **kw)
        assert np.isfinite(P).all() and np.isfinite(M).all(), (shape, "the recipe must stay finite")
        assert np.array_equal(zf, M[..., -1])
        lib_kw = {k: v for k, v in R.params(**kw).items() if k not in ("scale", "hop")}
        want, want_M = librosa_pcen(scale * S.astype(np.float64), hop_length=R.DEFAULTS["hop"], **lib_kw)
        # the smoother: relative 1e-14 of lfilter's (its transposed direct form II may round the same sum in another order)
        err = np.abs(M - want_M)
        assert (err <= 1e-14 * np.abs(want_M)).all(), (shape, float((err / np.maximum(np.abs(want_M), 1e-300)).max()))
        worst = max(worst, float((err / np.maximum(np.abs(want_M), 1e-300)).max()))
        # the compression: librosa's own expressions on the restatement's M give the restatement's bits
        u = np.float64(scale) * S.astype(np.float64)
        p = R.params(**kw)
        with np.errstate(divide="ignore", invalid="ignore"):
            sm = np.exp(-p["gain"] * (np.log(p["eps"]) + np.log1p(M / p["eps"])))
            if p["power"] == 0:
                direct = np.log1p(u * sm / p["bias"])
            elif p["bias"] == 0:
                direct = np.exp(p["power"] * (np.log(u) + np.log(sm)))
            else:
                direct = (p["bias"] ** p["power"]) * np.expm1(p["power"] * np.log1p(u * sm / p["bias"]))
        assert np.array_equal(direct, P), shape
        # and on lfilter's M they agree to rounding
        check_close(P, want, shape=S.shape, msg="%s %s" % (name, shape))
    print("smoother against lfilter: relative %.3g at most" % worst)


def test_the_textbook_form_is_not_the_definition():
    """(u / (eps + M)**gain + bias)**power - bias**power cancels on small outputs: it agrees in absolute terms only"""
    S = R.inputs(7, 3, 43, 321)
    p = R.params()
    P, M, _ = R.pcen(S)
    u = S.astype(np.float64)
    textbook = (u / (p["eps"] + M) ** p["gain"] + p["bias"]) ** p["power"] - p["bias"] ** p["power"]
    assert (np.abs(textbook - P) <= 1e-12 + 1e-9 * np.abs(P)).all()
    small = (P > 0) & (P < 1e-12)
    assert small.any() and (np.abs(textbook[small] - P[small]) > 1e-3 * P[small]).any()


def test_coefficient_and_start():
    assert R.coefficient(b=0.25) == 0.25
    T = 0.4 * 22050 / 512
    assert R.coefficient() == (np.sqrt(1 + 4 * T * T) - 1) / (2 * T * T)
    S = R.inputs(3, 2, 5, 64)
    # M[-1] = u[0]: the first value of the smoother is a u[0] + s u[0]
    u, M, zf = R.smooth(S, 0.25, 3.0)
    assert np.array_equal(M[..., 0], 0.75 * u[..., 0] + 0.25 * u[..., 0])
    # a call continued from zf is the whole call
    _, head, z = R.smooth(S[..., :20], 0.25, 3.0)
    _, tail, z2 = R.smooth(S[..., 20:], 0.25, 3.0, zi=z)
    assert np.array_equal(np.concatenate([head, tail], axis=-1), M) and np.array_equal(z2, zf)
