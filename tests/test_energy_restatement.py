"""The numpy restatements of the energy features against the reference's golden vectors (librosa 0.11, energy_goldens.ml) and
against each other.  No GPU.

  * the reference-order restatement meets every golden at the reference's own tolerances (energy_goldens.ml:14-21, 52-110);
  * the kernel-order rms differs from it by at most (frame_length + 4) * 2^-53 relative: two orders of a sum of frame_length
    non-negative terms are each within (frame_length - 1) * 2^-53 of the exact sum (relative, to first order), the root halves
    the sum of the two, and the division and the root add one rounding each on either side;
  * the kernel-order zero-crossing rate equals the reference-order one exactly (integer counts)."""
import numpy as np
import pytest

from conftest import F32_ATOL, F32_RTOL, F64_ATOL, F64_RTOL, check_close, golden_cases

import energy_restatement as R

GEOMETRIES = [(2048, 512, 5000), (16, 4, 700), (15, 7, 64), (8, 11, 60), (1, 3, 20), (9, 2, 50), (2048, 512, 3), (2048, 512, 1),
              (200, 64, 900), (96, 96, 500)]


def tolerances(dtype, strict=False):
    if dtype == "float32":
        return dict(rtol=F32_RTOL, atol=F32_ATOL)
    return {} if strict else dict(rtol=F64_RTOL, atol=F64_ATOL)


@pytest.mark.parametrize("case", golden_cases("energy", "rms"))
def test_rms_goldens(case):
    p = case["params"]
    got = R.rms_reference(R.golden_signal(p), p["frame_length"], p["hop"])
    assert got.dtype == np.dtype(p["dtype"])
    check_close(got.reshape(case["shape"]), case["values"], case["shape"], msg=case["name"], **tolerances(p["dtype"]))


@pytest.mark.parametrize("case", golden_cases("energy", "zero_crossing_rate"))
def test_zero_crossing_rate_goldens(case):
    p = case["params"]
    kw = {} if p["threshold"] is None else dict(threshold=p["threshold"])
    got = R.zcr_reference(R.golden_signal(p), p["frame_length"], p["hop"], **kw)
    check_close(got.reshape(case["shape"]), case["values"], case["shape"], msg=case["name"], **tolerances(p["dtype"], strict=True))


@pytest.mark.parametrize("case", golden_cases("energy", "rms_spectrogram"))
def test_rms_of_spectrogram_goldens(case):
    p = case["params"]
    s = R.golden_spectrogram(p)
    for f in (R.rms_of_spectrogram_reference, R.rms_of_spectrogram_ordered):
        got = f(s, p["frame_length"])
        check_close(got.reshape(case["shape"]), case["values"], case["shape"], msg=case["name"], **tolerances(p["dtype"]))


def test_the_23_goldens_are_all_here():
    assert sum(len(golden_cases("energy", n)) for n in ("rms", "rms_spectrogram", "zero_crossing_rate")) == 23


def test_frame_grid():
    assert [R.frames(n, fl, hop) for fl, hop, n in ((16, 4, 100), (15, 7, 64), (8, 11, 60), (1, 3, 20), (2048, 512, 0))] == [26, 10, 6, 7, 0]
    assert R.frames(1, 2048, 512) == 1 and R.frames(3, 2048, 512) == 1


@pytest.mark.parametrize("frame_length,hop,n", GEOMETRIES)
def test_kernel_order_rms_within_the_bound_of_the_reference_order(frame_length, hop, n):
    x = R.decades(frame_length * 31 + hop, 3, n, np.float64)
    want, got = R.rms_reference(x, frame_length, hop), R.rms_kernel_order(x, frame_length, hop)
    assert got.shape == want.shape == (3, 1, R.frames(n, frame_length, hop))
    bound = (frame_length + 4) * 2.0 ** -53
    worst = float(np.max(np.abs(got - want) / np.where(want > 0, want, 1.0)))
    assert worst <= bound, "%.3g beyond %.3g" % (worst, bound)


@pytest.mark.parametrize("frame_length,hop,n", GEOMETRIES)
@pytest.mark.parametrize("threshold", [1e-10, 0.0, 0.3])
def test_kernel_order_zcr_equals_the_reference_order(frame_length, hop, n, threshold):
    x = np.random.default_rng(n).uniform(-1, 1, size=(3, n))
    for dtype in (np.float32, np.float64):
        want = R.zcr_reference(x.astype(dtype), frame_length, hop, threshold)
        assert np.array_equal(R.zcr_kernel_order(x.astype(dtype), frame_length, hop, threshold), want)
    if frame_length == 1:
        assert not want.any()


def test_the_order_matters_for_these_inputs():
    """the bit-for-bit tests on the device would show nothing if every order gave the same bits"""
    x = R.decades(7, 3, 5000, np.float64)
    assert not np.array_equal(R.rms_kernel_order(x), R.rms_reference(x))
