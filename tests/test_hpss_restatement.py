"""The numpy restatement of hpss.ml (tests/hpss_restatement.py) against the reference's own golden vectors
(soundml/test/hpss/vectors, committed repacked with the values untouched under tests/golden/hpss): this pins the yardstick the GPU tests
compare against at sizes the goldens do not reach.  Tolerances are the reference's (hpss_goldens.ml:29-35, tutils);
hard-mask cases are checked by exact agreement, no flipped cell."""
import numpy as np
import pytest

from conftest import F32_ATOL, F32_RTOL, F64_ATOL, F64_RTOL, check_close
from oracle import soundml_oracle as O

import hpss_restatement as R


def tolerances(params):
    return (F64_RTOL, F64_ATOL) if params["dtype"] == "float64" else (F32_RTOL, F32_ATOL)


def check_case(case, face, masks):
    p = case["params"]
    s = R.golden_spectrogram(p).astype(p["dtype"])
    got = R.component(p, face(s, **R.golden_arguments(p)))
    assert got.dtype == np.dtype(p["dtype"])
    if masks and p["power"] == "inf":
        flipped = int((got.astype(np.float64).reshape(-1) != np.asarray(case["values"])).sum())
        assert list(got.shape) == case["shape"] and flipped == 0, "%s: %d cells flipped" % (case["name"], flipped)
    else:
        rtol, atol = tolerances(p)
        check_close(got, case["values"], shape=case["shape"], rtol=rtol, atol=atol, msg=case["name"])


@pytest.mark.parametrize("case", R.golden_cases("hpss"))
def test_spectrogram_goldens(case):
    check_case(case, R.hpss_of_spectrogram, False)


@pytest.mark.parametrize("case", R.golden_cases("hpss_boundary"))
def test_boundary_goldens(case):
    check_case(case, R.hpss_of_spectrogram, False)


@pytest.mark.parametrize("case", R.golden_cases("hpss_masks"))
def test_mask_goldens(case):
    check_case(case, R.hpss_masks, True)


@pytest.mark.parametrize("case", R.golden_cases("hpss_effects"))
def test_effects_goldens(case):
    p = case["params"]
    c = O.stft_config(p["fft_size"], hop=p["hop"], pad="constant", pad_value=0.0)
    x = O.lcg_signal(p["length"], p["seed"]).astype(p["dtype"])
    pair = R.hpss(c, x, **R.golden_arguments(p))
    got = {"hpss": R.component(p, pair), "harmonic": pair[0], "percussive": pair[1]}[p["face"]]
    rtol, atol = tolerances(p)
    check_close(got, case["values"], shape=case["shape"], rtol=rtol, atol=atol, msg=case["name"])


def test_reflection_and_rank_conventions():
    assert R.refl(np.array([-1, 0, 8, 9, 10, -10, 18, -19]), 9).tolist() == [0, 0, 8, 8, 7, 8, 0, 0]
    line = np.array([[5.0, 1.0, 4.0, 2.0, 3.0]])
    # even kernel: window [i - 1, i] (left-biased), the UPPER of the two
    assert R.running_median(line, 2, -1).tolist() == [[5.0, 5.0, 4.0, 4.0, 3.0]]
    assert R.running_median(line, 3, -1).tolist() == [[5.0, 4.0, 2.0, 3.0, 3.0]]
