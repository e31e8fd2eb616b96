"""The numpy restatement of effects.ml (tests/effects_restatement.py) against the reference's own golden vectors
(soundml/test/pvoc/vectors, committed repacked with the values untouched under tests/golden/pvoc): this pins the yardstick
the GPU tests compare against on spectra the goldens do not hold.  Tolerances are the reference's (pvoc_goldens.ml:44, 63,
97-123): float64 cases at 1e-11 absolute, float32 cases at the house pair, the pitch cases at 4e-2 of the case's peak
(the resampler substitution: this library's single-stage Kaiser design against soxr)."""
import numpy as np
import pytest

from conftest import F32_ATOL, F32_RTOL, check_close
from soundml_amd import Resample

import effects_restatement as R


def replay(case, got, fraction=None):
    p = case["params"]
    assert got.dtype == np.dtype(p["dtype"])
    if fraction is not None:
        rtol, atol = 0.0, fraction * float(np.max(np.abs(case["values"])))
    elif p["dtype"] == "float64":
        rtol, atol = 0.0, R.FLOAT64_ATOL
    else:
        rtol, atol = F32_RTOL, F32_ATOL
    check_close(got, case["values"], shape=case["shape"], rtol=rtol, atol=atol, msg=case["name"])


@pytest.mark.parametrize("case", R.golden_cases("stretch"))
def test_stretch_goldens(case):
    p = case["params"]
    replay(case, R.time_stretch(R.golden_config(p), R.golden_signal(p), p["rate"]))


@pytest.mark.parametrize("case", R.golden_cases("pitchstretch"))
def test_pitchstretch_goldens(case):
    """The stretch stage of the pitch cases, at the very quotient den / num (the recorded rate is that quotient)."""
    p = case["params"]
    rate = float(p["den"]) / float(p["num"])
    assert rate == p["rate"]
    replay(case, R.time_stretch(R.golden_config(p), R.golden_signal(p), rate))


@pytest.mark.parametrize("case", R.golden_cases("locked"))
def test_locked_goldens(case):
    p = case["params"]
    replay(case, R.time_stretch(R.golden_config(p), R.golden_signal(p), p["rate"], locked=True))


@pytest.mark.parametrize("case", R.golden_cases("pitch"))
def test_pitch_goldens(case):
    """Every ratio plans under the bank budget (L = 1, 2, 2797, 1772, 3363): no case is skipped."""
    p = case["params"]
    resampler = Resample.Config.create(p["num"], p["den"])
    replay(case, R.pitch_shift(R.golden_config(p), R.golden_signal(p), (p["num"], p["den"]), resampler), fraction=R.PITCH_FRACTION)


def test_the_files_are_whole():
    assert [len(R.golden_cases(n)) for n in ("stretch", "pitchstretch", "pitch", "locked")] == [63, 11, 11, 3]
    assert {c.values[0]["params"]["num"] for c in R.golden_cases("pitch")} >= {1, 2}


def test_locking_conventions():
    # strict peaks among the neighbours a bin has; a plateau has none
    assert R.peaks_of(np.array([3.0, 1.0, 0.5, 1.0, 4.0, 1.0, 1.0])).tolist() == [0, 4]
    assert R.peaks_of(np.array([1.0, 1.0, 1.0])).tolist() == []
    # regions split at (kp + kp_next + 1) / 2: bin 2, equidistant from peaks 0 and 4, goes to the upper one
    phi = np.arange(7, dtype=np.float64) * 10.0
    ang = np.arange(7, dtype=np.float64)
    got = R.lock(phi, ang, np.array([0, 4]))
    assert got.tolist() == [0.0, 0.0 + 1.0, 40.0 - 2.0, 40.0 - 1.0, 40.0, 40.0 + 1.0, 40.0 + 2.0]


def test_lengths_round_half_even():
    assert [R.stretch_length(n, 2.0) for n in (5, 7, 0, 1)] == [2, 4, 0, 0]
    assert R.out_frames(0, 0.5) == 0 and R.out_frames(9, 2.0) == 5 and R.out_frames(9, 0.75) == 12
