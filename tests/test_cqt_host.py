"""Cqt.Config on the host (no device): the library's plan against the numpy restatement and the reference's support goldens,
the 0/1 chroma fold against chroma_fb.json, every Invalid_argument of ``create`` (cqt.ml:261-364) and the float64 rejection."""
import numpy as np
import pytest

from conftest import F64_ATOL, F64_RTOL, check_close
from soundml_amd import Chroma, Cqt, InvalidArgument, Resample, chroma_cqt

import cqt_restatement as R

PLANS = {
    "c1_84": dict(n_bins=84, sample_rate=22050),
    "c1_84_hop511": dict(n_bins=84, sample_rate=22050, hop=511),
    "bpo36_252": dict(n_bins=252, sample_rate=22050, bins_per_octave=36),
    "partial_90_hop256": dict(n_bins=90, sample_rate=22050, hop=256),
    "early_48_noscale": dict(n_bins=48, sample_rate=22050, scale=False),
    "one_bin": dict(n_bins=1, sample_rate=22050),
    "seven_bins": dict(n_bins=7, sample_rate=22050),
    "erb_kaiser_l2": dict(n_bins=84, sample_rate=22050, gamma="erb", window=("kaiser", 8.6), norm=2.0),
    "fixed20_tuned": dict(n_bins=84, sample_rate=22050, gamma=20.0, tuning=0.22, filter_scale=0.5),
    "sr44100_bkh": dict(n_bins=84, sample_rate=44100, window="blackman_harris"),
}


@pytest.mark.parametrize("name", sorted(PLANS))
def test_plan_matches_the_restatement(name):
    kw = PLANS[name]
    c, r = Cqt.Config.create(**kw), R.Config(**kw)
    assert (c.n_bins, c.bins_per_octave, c.sample_rate, c.hop, c.n_octaves, c.early) == \
        (r.n_bins, r.bins_per_octave, r.sample_rate, r.hop, r.n_octaves, r.early)
    assert c.octaves == [(o.first, o.count, o.n_fft, o.hop, o.halvings) for o in r.octaves]
    # the same float64 expressions in the same order: equal to the last bit
    assert np.array_equal(Cqt.frequencies(np.float64, c), r.freqs)
    assert np.array_equal(Cqt.filter_lengths(np.float64, c), r.lengths)
    assert c.cutoff == r.cutoff
    assert np.array_equal(c.divisors(), r.divisors if r.divisors is not None else np.ones(r.n_bins))
    assert Cqt.frequencies(np.float32, c).dtype == np.float32
    assert c.latency == r.latency(Resample.Config.create(2, 1, "high").latency)
    for n in (0, 1, 2, 100, 255, 256, 511, 512, 513, 4096, 8192, 22050):
        assert Cqt.frames(c, n) == R.frames(r, n)
    # the taps: two radix-2 transforms here, numpy's there
    for i, o in enumerate(r.octaves):
        want = o.taps()
        assert np.max(np.abs(c.taps(i) - want)) <= 1e-13 * np.max(np.abs(want))


def test_documented_latencies():
    """cqt.mli:222-227."""
    assert Cqt.Config.create(84, 22050).latency == 20099
    assert Cqt.Config.create(84, 22050, hop=511).latency == 8192


def support(kind):
    return [pytest.param(c, id=c["name"]) for c in R.golden_cases("cqt", "cqt_support") if c["params"]["kind"] in kind]


@pytest.mark.parametrize("case", support(("frequencies", "filter_lengths", "cutoff")))
def test_support_values(case):
    c = Cqt.Config.create(**R.golden_kwargs(case["params"]))
    kind = case["params"]["kind"]
    got = Cqt.frequencies(np.float64, c) if kind == "frequencies" else \
        Cqt.filter_lengths(np.float64, c) if kind == "filter_lengths" else np.array([c.cutoff])
    check_close(got, case["values"], shape=case["shape"], rtol=F64_RTOL, atol=F64_ATOL, msg=case["name"])


@pytest.mark.parametrize("case", support(("early",)))
def test_support_early(case):
    """cqt_goldens.ml:225-237: read back from the frame grid, and the accessor."""
    c = Cqt.Config.create(**R.golden_kwargs(case["params"]))
    n = next(n for n in range(1, c.hop + 1) if Cqt.frames(c, n) >= 2)
    assert np.log2(float(c.hop + 1 - n)) == case["values"][0] == float(c.early)


@pytest.mark.parametrize("case", support(("nyquist",)))
def test_support_nyquist(case):
    try:
        Cqt.Config.create(**R.golden_kwargs(case["params"]))
        accepted = 1.0
    except InvalidArgument:
        accepted = 0.0
    assert accepted == case["values"][0]


@pytest.mark.parametrize("case", [pytest.param(c, id=c["name"]) for c in R.golden_cases("chroma", "chroma_fb")
                                  if c["params"]["kind"] == "cqt_projection"])
def test_cqt_projection(case):
    """chroma_goldens.ml:142-150: the assignment is exactly zero or one."""
    p = case["params"]
    c = Cqt.Config.create(n_bins=p["n_bins"], sample_rate=p["sample_rate"], fmin=p["fmin"], bins_per_octave=p["bins_per_octave"],
                          tuning=p["tuning"], hop=p["hop"])
    got = Chroma.cqt_projection(np.float64, c, n_chroma=p["n_chroma"])
    assert list(got.shape) == case["shape"]
    assert np.array_equal(got.reshape(-1), np.asarray(case["values"]))
    assert Chroma.cqt_projection(np.float32, c, n_chroma=p["n_chroma"]).dtype == np.float32


INVALID = [
    (dict(n_bins=0, sample_rate=22050), "create: cannot use n_bins = 0 (n_bins must be at least 1)"),
    (dict(n_bins=12, sample_rate=22050, bins_per_octave=0), "create: cannot use bins_per_octave = 0 (bins_per_octave must be at least 1)"),
    (dict(n_bins=12, sample_rate=22050, hop=0), "create: cannot use hop = 0 (hop must be at least 1)"),
    (dict(n_bins=12, sample_rate=0), "create: cannot use sample_rate = 0 (sample_rate must be at least 1)"),
    (dict(n_bins=12, sample_rate=22050, fmin=0.0), "create: cannot use fmin = 0 (fmin must be finite and positive)"),
    (dict(n_bins=12, sample_rate=22050, fmin=float("nan")), "create: cannot use fmin = nan (fmin must be finite and positive)"),
    (dict(n_bins=12, sample_rate=22050, tuning=float("inf")), "create: cannot use tuning = inf (tuning must be finite)"),
    (dict(n_bins=12, sample_rate=22050, filter_scale=-1.0), "create: cannot use filter_scale = -1 (filter_scale must be finite and positive)"),
    (dict(n_bins=12, sample_rate=22050, norm=0.0), "create: cannot use norm = 0 (norm must be finite and positive)"),
    (dict(n_bins=12, sample_rate=22050, gamma=-1.0), "create: cannot use gamma = -1 (gamma must be finite and non-negative)"),
    (dict(n_bins=12, sample_rate=22050, window=("kaiser", -1.0)),
     "create: cannot use a kaiser window with beta -1 (beta must be finite and non-negative)"),
    (dict(n_bins=12, sample_rate=22050, window=("tukey", 1.5)), "create: cannot use a tukey window with taper 1.5 (taper must lie in [0, 1])"),
    (dict(n_bins=5000, sample_rate=22050, fmin=1e300),
     "create: cannot place 5000 bins from 1e+300 Hz at 12 bins per octave (the frequency ladder overflows)"),
    (dict(n_bins=102, sample_rate=22050),
     "create: cannot place 102 bins from 32.7032 Hz at a sample rate of 22050 Hz (bin 101, centred at 11175.3 Hz, reaches 11659 Hz, "
     "above the Nyquist frequency 11025)"),
    # a large fixed bandwidth offset shortens the filters without raising the cutoff past Nyquist
    (dict(n_bins=12, sample_rate=22050, fmin=100.0, gamma=10000.0, filter_scale=0.2),
     "create: cannot resolve 12 bins from 100 Hz with filter_scale = 0.2 (the filters of octave 0 span less than one sample)"),
]


@pytest.mark.parametrize("kw,message", INVALID, ids=[m.split("(")[0].strip().replace(" ", "_")[:60] + str(i) for i, (_, m) in enumerate(INVALID)])
def test_create_rejects(kw, message):
    with pytest.raises(InvalidArgument) as e:
        Cqt.Config.create(**kw)
    assert str(e.value) == message
    with pytest.raises(ValueError) as r:     # the restatement words it the same way
        R.Config(**kw)
    assert str(r.value) == message


def test_create_rejects_unknown_names():
    for kw in (dict(gamma="loud"), dict(window="boxcar"), dict(pad="wrap")):
        with pytest.raises(InvalidArgument):
            Cqt.Config.create(12, 22050, **kw)


def test_frames_rejects_negative_lengths():
    with pytest.raises(InvalidArgument, match="frames: cannot analyse a signal of length -3"):
        Cqt.frames(Cqt.Config.create(12, 22050), -3)


def test_float64_audio_is_rejected():
    """DEVIATION: float32 audio only, as Resample.apply."""
    c = Cqt.Config.create(12, 22050, fmin=1500.0)
    x = np.zeros((2, 1024), dtype=np.float64)
    for call in (lambda: Cqt.transform(c, x), lambda: Cqt.power_spectrum(c, x), lambda: chroma_cqt(c, x)):
        with pytest.raises(InvalidArgument, match="cannot analyse float64 audio"):
            call()
    with pytest.raises(InvalidArgument, match="transform: cannot analyse a rank-zero tensor"):
        Cqt.transform(c, np.float32(1.0))


def test_of_cqt_conditions_need_no_device():
    """chroma.ml:347-381, in the reference's order: the norm, the resolution, the rank, the bin count; then the empty result."""
    c = Cqt.Config.create(84, 22050)
    s = np.zeros((60, 3), dtype=np.float32)
    with pytest.raises(InvalidArgument, match=r"of_cqt: cannot normalise in the -1-norm"):
        Chroma.of_cqt(c, s, norm=-1.0)
    with pytest.raises(InvalidArgument) as e:
        Chroma.of_cqt(c, s, n_chroma=5)
    assert str(e.value) == ("of_cqt: cannot fold 12 bins per octave onto 5 chroma bands (bins_per_octave must be an integer multiple "
                            "of n_chroma)")
    with pytest.raises(InvalidArgument) as e:
        Chroma.cqt_projection(np.float64, c, n_chroma=24)
    assert str(e.value) == ("cqt_projection: cannot fold 12 bins per octave onto 24 chroma bands (bins_per_octave must be an integer "
                            "multiple of n_chroma)")
    with pytest.raises(InvalidArgument, match="cqt_projection: cannot build 0 chroma bands"):
        Chroma.cqt_projection(np.float64, c, n_chroma=0)
    with pytest.raises(InvalidArgument, match="of_cqt: cannot project a rank-1 tensor"):
        Chroma.of_cqt(c, np.zeros(84, dtype=np.float32))
    with pytest.raises(InvalidArgument) as e:
        Chroma.of_cqt(c, s)
    assert str(e.value) == "of_cqt: cannot project 60 constant-Q bins through a configuration of 84 bins"
    assert Chroma.of_cqt(c, np.zeros((84, 0), dtype=np.float64)).shape == (12, 0)      # chroma_props.ml:265-267
    assert Cqt.transform(c, np.zeros((2, 0), dtype=np.float32)).shape == (2, 84, 0)
    assert Cqt.power_spectrum(c, np.zeros((0, 512), dtype=np.float32)).shape == (0, 84, 2)


def test_config_equality_and_repr():
    a, b = Cqt.Config.create(84, 22050), Cqt.Config.create(84, 22050)
    assert a == b and a != Cqt.Config.create(84, 22050, hop=256)
    assert repr(a) == ("cqt(n_bins=84, bins_per_octave=12, sample_rate=22050, fmin=32.7032, hop=512, gamma=constant_q, tuning=0, "
                       "filter_scale=1, norm=1, window=hann, scale=true, pad=constant(0))")
