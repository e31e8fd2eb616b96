"""The numpy restatement of contrast.ml / onset.ml (tests/contrast_onset_restatement.py) against the reference's own golden
vectors (soundml/test/onset/vectors, committed unchanged under tests/golden/onset): this pins the yardstick the GPU tests
compare against at sizes the goldens do not reach.  Tolerances are the reference's (onset_goldens.ml:24-32, tutils): float64
1e-9 / 1e-12 in the linear domain and 1e-9 / 1e-9 in the logarithmic one, float32 1e-6 / 1e-7 and 1e-4 / 1e-4."""
import numpy as np
import pytest

from conftest import F32_ATOL, F32_RTOL, F64_ATOL, F64_RTOL, check_close, golden_cases
from oracle import soundml_oracle as O

import contrast_onset_restatement as R

LOG64_ATOL, LOG32_RTOL, LOG32_ATOL = 1e-9, 1e-4, 1e-4


def tolerances(dtype, linear):
    if dtype == "float64":
        return F64_RTOL, (F64_ATOL if linear else LOG64_ATOL)
    return (F32_RTOL, F32_ATOL) if linear else (LOG32_RTOL, LOG32_ATOL)


def golden_input(p):
    c = O.stft_config(p["fft_size"], hop=p["hop"], alignment=p["alignment"])
    return c, R.signal(p["length"], envelope=p["envelope"], silence_tail=p["silence_tail"]).astype(p["dtype"])


@pytest.mark.parametrize("case", golden_cases("onset", "spectral_contrast"))
def test_contrast_goldens(case):
    p = case["params"]
    c, x = golden_input(p)
    got = R.spectral_contrast(c, x, p["sample_rate"], p["n_bands"], p["f_min"], p["quantile"], p["linear"])
    assert got.dtype == np.dtype(p["dtype"])
    rtol, atol = tolerances(p["dtype"], p["linear"])
    check_close(got, case["values"], shape=case["shape"], rtol=rtol, atol=atol, msg=case["name"])


@pytest.mark.parametrize("case", golden_cases("onset", "onset_strength"))
def test_onset_goldens(case):
    p = case["params"]
    c, x = golden_input(p)
    got = R.onset_strength(c, O.mel_config(p["n_mels"], p["sample_rate"], p["fft_size"]), x, p["lag"])
    assert got.dtype == np.dtype(p["dtype"])
    rtol, atol = tolerances(p["dtype"], False)
    check_close(got, case["values"], shape=case["shape"], rtol=rtol, atol=atol, msg=case["name"])


def test_the_two_default_plans():
    assert R.plan(6, 200.0, 0.02, 22050, 2048) == [(0, 18, 1), (18, 19, 1), (37, 37, 1), (74, 74, 2), (148, 149, 3), (297, 297, 6),
                                                   (594, 431, 9)]
    assert R.plan(6, 200.0, 0.02, 48000, 2048)[-1] == (273, 752, 15)
    assert [R.plan(6, 200.0, q, 22050, 2048)[-1][2] for q in (0.0375, 0.04, 0.5)] == [16, 17, 216]
