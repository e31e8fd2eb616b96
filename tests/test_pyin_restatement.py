"""pYIN without a device: the host tables against scipy's pins (tests/golden/pitch/pyin_pins.json, tools/gen_pyin_pins.py) and
against numpy's formulas, and the restatement (tests/pyin_restatement.py) against what it must be: a Viterbi decoder, with the stated
ties, alive across a jump wider than the band, and a pitch tracker that finds harmonic tones.

The pins' gate: the largest absolute difference of beta and of Z * E from the JSON was measured at 1.6653345369377348e-15 (beta at
(2, 18), 100 thresholds; Z * E differs by 3.4e-21 at most); the gate is 4 times that, and the figure itself must stay below 1e-12
(the cdf values are at most 1: a few-ulp evaluation)."""
import json
import math
import os

import numpy as np
import pytest

from soundml_amd import Pitch

import pitch_restatement as P
import pyin_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEASURED = 1.6653345369377348e-15
GATE = 4 * MEASURED


def pins():
    with open(os.path.join(ROOT, "tests", "golden", "pitch", "pyin_pins.json")) as fh:
        return json.load(fh)


def test_tables_against_the_pins():
    assert MEASURED < 1e-12
    worst = 0.0
    for p in pins()["beta"]:
        t = Pitch.pyin_tables(65, 2093, n_thresholds=p["n"], beta_parameters=(p["a"], p["b"]))
        assert t["beta"].shape == (p["n"],) and np.array_equal(t["thr"], np.arange(p["n"] + 1) / float(p["n"]))
        worst = max(worst, float(np.abs(t["beta"] - np.array(p["values"])).max()))
    for p in pins()["boltzmann"]:
        t = Pitch.pyin_tables(65, 2093, boltzmann_parameter=p["lambda"])
        assert t["E"].shape == (t["maxr"],) and t["Z"].shape == (t["maxr"] + 1,) and p["N"] <= t["maxr"]
        worst = max(worst, float(np.abs(t["Z"][p["N"]] * t["E"][:p["N"]] - np.array(p["values"])).max()))
    print("largest absolute difference from the pins: %r" % worst)
    assert worst <= GATE
    for p in pins()["bins"]:
        assert Pitch.pyin_bins(p["fmin"], p["fmax"], p["resolution"]) == p["n_bins"]
    for p in pins()["half_width"]:
        assert Pitch.pyin_half_width(p["sample_rate"], p["hop"], p["resolution"], p["max_transition_rate"]) == p["h"]


def ulps(got, want):
    return float(np.max(np.abs(got - want) / np.spacing(np.abs(want))))


@pytest.mark.parametrize("fmin,fmax,sr,hop,resolution,rate", [(65.0, 2093.0, 22050, 512, 0.1, 35.92), (100.0, 1000.0, 8000, 64, 0.1, 35.92),
                                                            (400.0, 500.0, 8000, 64, 0.1, 35.92), (100.0, 1000.0, 8000, 64, 0.5, 1.0)])
def test_tables_against_numpy(fmin, fmax, sr, hop, resolution, rate):
    t = Pitch.pyin_tables(fmin, fmax, sample_rate=sr, frame_length=256 if sr == 8000 else 2048, hop=hop, resolution=resolution,
                          max_transition_rate=rate)
    bps = math.ceil(1.0 / resolution)
    nb, h = t["n_bins"], t["h"]
    assert nb == int(math.floor(12 * bps * math.log2(fmax / fmin))) + 1 and h == (round(rate * 12.0 * hop / sr) * bps) // 2
    assert ulps(t["freq"], fmin * np.exp2(np.arange(nb) / (12.0 * bps))) <= 4
    assert ulps(t["edge"], fmin * np.exp2((np.arange(1, nb) - 0.5) / (12.0 * bps))) <= 4
    assert np.all(np.diff(t["edge"]) > 0) and np.all(t["freq"][:-1] < t["edge"]) and np.all(t["edge"] < t["freq"][1:])
    tri = 1.0 - np.abs(np.arange(2 * h + 1) - h) / float(h + 1)
    assert t["tri"].shape == (2 * h + 1,) and ulps(t["tri"], tri) <= 4
    sums = np.array([sum(tri[j - i + h] for j in range(max(0, i - h), min(nb - 1, i + h) + 1)) for i in range(nb)])
    assert ulps(t["rs"], 1.0 / sums) <= 4
    assert np.array_equal(t["E"], np.exp(-2.0 * np.arange(t["maxr"]))) or ulps(t["E"], np.exp(-2.0 * np.arange(t["maxr"]))) <= 4


# ---- the decoder is a Viterbi decoder --------------------------------------------------------------------------------------------

def band(nb, h):
    tri = np.zeros(2 * h + 1)
    rs = np.zeros(nb)
    tri[:] = 1.0 - np.abs(np.arange(2 * h + 1) - h) / float(h + 1)
    for i in range(nb):
        s = 0.0
        for j in range(max(0, i - h), min(nb - 1, i + h) + 1):
            s = s + tri[j - i + h]
        rs[i] = 1.0 / s
    return tri, rs


def sparse_observation(seed, nb, h, T):
    """a few voiced candidates per frame, each within h of one of the frame before; voiced_prob < 1 in every frame"""
    rng = np.random.default_rng(seed)
    obs = np.zeros((2 * nb, T))
    near = [int(rng.integers(0, nb))]
    for t in range(T):
        count = int(rng.integers(1, 4))
        bins = sorted({int(np.clip(near[int(rng.integers(0, len(near)))] + rng.integers(-h, h + 1), 0, nb - 1)) for _ in range(count)})
        mass = rng.uniform(0.05, 0.9)
        share = rng.dirichlet(np.ones(len(bins))) * mass
        obs[bins, t] = share
        obs[nb:, t] = (1.0 - obs[:nb, t].sum()) / nb
        near = bins
    return obs


def log_viterbi(obs, tri, rs, switch_prob):
    """a dense log-domain decode: log of the same B and of the dense kron transition; (the optimum, log B, log A, log p_init)"""
    S, T = obs.shape
    nb, h = S // 2, (tri.size - 1) // 2
    pitch = np.zeros((nb, nb))
    for i in range(nb):
        for j in range(max(0, i - h), min(nb - 1, i + h) + 1):
            pitch[i, j] = tri[j - i + h] * rs[i]
    voicing = np.array([[1.0 - switch_prob, switch_prob], [switch_prob, 1.0 - switch_prob]])
    with np.errstate(divide="ignore"):
        logA = np.log(np.kron(voicing, pitch))
        logB = np.log(np.maximum(obs, R.FLOOR))
        logp = np.log(np.concatenate([np.zeros(nb), np.full(nb, 1.0 / nb)]))
    score = logp + logB[:, 0]
    for t in range(1, T):
        score = np.max(score[:, None] + logA, axis=0) + logB[:, t]
    return float(score.max()), logB, logA, logp


def path_score(states, logB, logA, logp):
    total = logp[states[0]] + logB[states[0], 0]
    for t in range(1, len(states)):
        total = total + logA[states[t - 1], states[t]] + logB[states[t], t]
    return float(total)


@pytest.mark.parametrize("seed,nb,h,T,switch_prob", [(1, 61, 10, 80, 0.01), (2, 61, 10, 80, 0.3), (3, 23, 30, 40, 0.01), (4, 40, 0, 30, 0.05),
                                                     (5, 17, 3, 60, 0.5)])
def test_the_decoder_is_a_viterbi_decoder(seed, nb, h, T, switch_prob):
    """by score, not by index: the restated path's log-probability is within 1e-9 of the dense optimum (sums of order 1e2 to 1e3 round
    at about 1e-13; a wrong step costs at least a factor switch_prob or a triangle ratio)"""
    tri, rs = band(nb, h)
    obs = sparse_observation(seed, nb, h, T)
    assert np.all(obs[:nb].sum(axis=0) < 1.0)
    states = R.decode(obs, tri, rs, switch_prob)
    best, logB, logA, logp = log_viterbi(obs, tri, rs, switch_prob)
    got = path_score(states, logB, logA, logp)
    print("seed %d: restated path %.12f, dense optimum %.12f" % (seed, got, best))
    assert np.isfinite(best) and abs(got - best) <= 1e-9


# ---- crafted cases (tests/test_gpu_pyin.py runs the same observations through the device) ------------------------------------------

def test_two_equal_candidates_keep_the_lower_bin():
    obs, h = R.crafted_equal_candidates()
    nb = obs.shape[0] // 2
    states = R.decode(obs, *band(nb, h), 0.01)
    assert states.tolist() == [nb + 8] + [8] * (obs.shape[1] - 1)


def test_a_jump_beyond_the_band_survives_through_the_floor():
    obs, h = R.crafted_jump()
    nb = obs.shape[0] // 2
    states, delta = R.decode(obs, *band(nb, h), 0.01, return_delta=True)
    assert np.all(obs[:nb].sum(axis=0) == 1.0) and abs(15 - 2) > h
    assert delta.max() > 0.0 and np.isfinite(delta).all()                      # never an all-zero frame
    assert np.all(states[2:] == 15) and np.all(states[1:] < nb) and states[0] >= nb     # p_init is zero on the voiced states
    assert np.all(np.abs(np.diff(states[1:] % nb)) <= h)


@pytest.mark.parametrize("T", [1, 2])
def test_one_and_two_frames(T):
    obs, h = R.crafted_short(T)
    nb = obs.shape[0] // 2
    states = R.decode(obs, *band(nb, h), 0.01)
    best, logB, logA, logp = log_viterbi(obs, *band(nb, h), 0.01)
    assert states.shape == (T,) and abs(path_score(states, logB, logA, logp) - best) <= 1e-9
    if T == 1:
        assert states[0] == nb + int(np.argmax(obs[nb:, 0]))


def kw():
    return dict(fmin=65.0, fmax=2093.0, sample_rate=22050, frame_length=2048, hop=512)


def test_silence_is_unvoiced():
    tab = Pitch.pyin_tables(**kw())
    f0, flag, prob = R.pyin(np.zeros((1, 4096), np.float32), tab=tab, **kw())
    assert np.all(flag == 0.0) and np.all(np.isnan(f0)) and flag.dtype == np.float32 and flag.shape == (1, 1, 9)
    assert np.all(prob == 0.0)                   # d' = 1 everywhere: one trough at pmax that no threshold reaches, and no share
    f0 = R.pyin(np.zeros((1, 4096), np.float32), tab=tab, fill_na=None, **kw())[0]
    assert np.all(np.isin(f0, tab["freq"].astype(np.float32)))


@pytest.mark.parametrize("pitch", [82.41, 220.0, 440.0, 987.77])
def test_tones(pitch):
    """interior frames are voiced and f0 is within 10 cents of the pitch (half a bin is 5 cents; yin's 1e-3 is 1.7 cents)"""
    tab = Pitch.pyin_tables(**kw())
    f0, flag, prob = R.pyin(P.harmonic_tone(pitch, 8192, 22050, np.float64)[None], tab=tab, **kw())
    inner = slice(3, -3)
    assert np.all(flag[0, 0, inner] == 1.0) and np.all(prob[0, 0, inner] > 0.5)
    cents = 1200.0 * np.abs(np.log2(f0[0, 0, inner] / pitch))
    print("%g Hz: at most %.3f cents off" % (pitch, cents.max()))
    assert np.all(cents <= 10.0)
