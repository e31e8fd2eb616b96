"""Loudness without a device: the host-built tables against BS.1770-4's printed table and the numpy formulas, and the numpy
restatement (tests/loudness_restatement.py, the gate of the GPU tests) against the EBU Tech 3341 compliance signals at the
document's own tolerances.  The signals run at full length: cut to a tenth the restatement misses by 0.19 LU."""
import json
import os

import numpy as np
import pytest

from soundml_amd import Loudness

import loudness_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PINS = json.load(open(os.path.join(ROOT, "tests", "golden", "loudness", "pins.json")))


def test_k_weighting_at_48000_is_the_printed_table():
    sos = Loudness.k_weighting(48000)
    assert sos.shape == (2, 6) and sos.dtype == np.float64
    assert np.abs(sos - np.array(PINS["sos"])).max() <= 1e-12
    assert np.all(sos[:, 3] == 1.0) and np.array_equal(sos[1, :3], [1.0, -2.0, 1.0])


@pytest.mark.parametrize("rate", [44100, 22050, 96000, 8000])
def test_k_weighting_is_the_formula(rate):
    assert np.abs(Loudness.k_weighting(rate) - R.k_weighting(rate)).max() <= 1e-12


def test_true_peak_taps_are_the_formula():
    h = Loudness.true_peak_taps()
    assert h.shape == (49,) and h.dtype == np.float64
    assert np.abs(h - R.taps()).max() <= 1e-15
    assert abs(h.sum() - 4.0) <= 1e-14 and np.array_equal(h, h[::-1])


def test_constants():
    assert Loudness.ABSOLUTE_GATE == R.E_ABS == 10.0 ** ((PINS["absolute_gate_lufs"] - PINS["offset"]) / 10.0)
    assert tuple(Loudness.SURROUND_5_0) == tuple(PINS["surround_5_0"]) == R.SURROUND_5_0
    for rate in (48000, 44100, 22050, 11025, 8000):
        assert Loudness.step(rate) == R.step(rate) == (rate + 5) // 10 >= 256
        for n in (0, 4 * R.step(rate) - 1, 4 * R.step(rate), 5 * R.step(rate) - 1, 5 * R.step(rate), 123457):
            assert Loudness.blocks(rate, n) == R.blocks(rate, n)


@pytest.mark.parametrize("case", sorted(R.EBU))
def test_restatement_meets_ebu_3341(case):
    """integrated loudness of cases 1-6 within the document's +-0.1 LU"""
    _, weights, want = R.EBU[case]
    x = R.ebu_signal(case)
    got = float(R.measure(x[None], R.EBU_RATE, weights).integrated[0])
    print("EBU Tech 3341 case %d: %.4f LUFS (expected %.1f)" % (case, got, want))
    assert abs(got - want) <= 0.1


@pytest.mark.parametrize("k", range(len(R.TONES)))
def test_restatement_true_peak_meets_ebu_3341(k):
    """the faded tones within +0.2 / -0.4 dB of their true peak, with the library's taps"""
    want = R.TONES[k][3]
    got = 20.0 * np.log10(R.true_peak(R.tone(k)[None], Loudness.true_peak_taps())[0])
    print("tone %d: %.4f dBTP (expected %.1f), sample peak %.2f dBFS" % (k, got, want, 20.0 * np.log10(np.abs(R.tone(k)).max())))
    assert want - 0.4 <= got <= want + 0.2


def test_the_gating_clip_exercises_both_gates_with_a_margin():
    m = R.measure(R.gating_clip(), 48000)
    e = m.e[0]
    first, both, _ = R.gates(e)
    assert (~first).sum() >= 1 and (first & ~both).sum() >= 1 and both.sum() >= 1
    relative = 0.1 * R.serial_mean(e[first])
    for threshold in (R.E_ABS, relative):
        ratio = e / threshold
        assert not np.any((ratio > 1 / 1.001) & (ratio < 1.001))
