"""The numpy restatement of cqt.ml (tests/cqt_restatement.py) against the reference's own golden vectors
(soundml/test/cqt/vectors and the constant-Q rows of soundml/test/chroma/vectors, committed repacked under tests/golden, values untouched):
this pins the yardstick the device tests compare against on signals and plans the goldens do not hold.  Tolerances are the
reference's (cqt_goldens.ml:27-47), fractions of the case peak max|expected| plus rtol 1e-5: 1e-6 for float64 cases that
never decimate, 5e-6 for their float32 twins, 6e-4 for every case that decimates (this library's single-stage Kaiser 2:1
design against soxr_hq).  The decimator of those cases is the sparse polyphase stage of effects_restatement on the prototype
that Resample.Config.create(2, 1, "high") reports."""
import numpy as np
import pytest

from conftest import F64_ATOL, F64_RTOL, check_close
from soundml_amd import Resample

import cqt_restatement as R
from effects_restatement import resample_stage


def cases(suite, name, kind=None):
    return [pytest.param(c, id=c["name"]) for c in R.golden_cases(suite, name) if kind is None or c["params"]["kind"] in kind]


@pytest.fixture(scope="module")
def halver():
    half = Resample.Config.create(2, 1, "high")
    proto, (l, m), k = half.prototype(), half.rate, half.latency
    assert (l, m) == (1, 2) and proto.shape == (2 * k * l + 1,)
    return lambda y: resample_stage(proto, l, m, k, y)


def replay(case, decimate, fraction64, fraction32):
    p = case["params"]
    c = R.Config(**R.golden_kwargs(p))
    x = R.golden_signal(p)
    fraction = fraction64
    if p["dtype"] == "float32":   # the signal quantised to float32 against a float64 reference (cqt_goldens.ml:184-188)
        x, fraction = x.astype(np.float32).astype(np.float64), fraction32
    got = R.power_spectrum(c, x, decimate, 1.0)
    peak = float(np.max(np.abs(case["values"])))
    check_close(got, case["values"], shape=case["shape"], rtol=R.RTOL, atol=fraction * peak, msg=case["name"])
    return c


@pytest.mark.parametrize("case", cases("cqt", "cqt_tight"))
def test_tight_goldens(case):
    replay(case, R.no_decimation, R.TIGHT_ATOL, R.TIGHT32_ATOL)


@pytest.mark.parametrize("case", cases("cqt", "cqt_wide"))
def test_wide_goldens(case, halver):
    c = replay(case, halver, R.WIDE_ATOL, R.WIDE_ATOL)
    assert c.early > 0 or any(o.hop % 2 == 0 for o in c.octaves[:-1])   # every case of this file decimates


def test_the_taps_are_the_kernel(halver):
    """K @ rfft(frame) = sum_n frame[n] g[b, n]: the form the device consumes, on every octave of the odd-hop 84-bin plan."""
    c = R.Config(84, 22050, hop=511)
    assert [o.n_fft for o in c.octaves] == [256, 512, 1024, 2048, 4096, 8192, 16384]
    x = R.golden_signal(dict(length=8192, signal="lcg", sample_rate=22050))
    count = R.frames(c, 8192)
    for o in c.octaves:
        want = np.matmul(o.kernel, R.octave_spectrum(o, x, count, "constant", 0.0))
        xp = R.padded(x, o.n_fft // 2, o.n_fft // 2, "constant", 0.0)
        got = np.stack([o.taps() @ xp[p * o.hop:p * o.hop + o.n_fft] for p in range(count)], axis=1)
        assert np.max(np.abs(got - want)) <= 1e-12 * np.max(np.abs(want))


@pytest.mark.parametrize("case", cases("cqt", "cqt_support", ("frequencies", "filter_lengths", "cutoff")))
def test_support_values(case):
    """cqt_goldens.ml:201-219: closed-form doubles at the default float64 grade."""
    c = R.Config(**R.golden_kwargs(case["params"]))
    got = {"frequencies": c.freqs, "filter_lengths": c.lengths, "cutoff": np.array([c.cutoff])}[case["params"]["kind"]]
    check_close(got, case["values"], shape=case["shape"], rtol=F64_RTOL, atol=F64_ATOL, msg=case["name"])


def early_of(c):
    """cqt_goldens.ml:225-232: the early-decimation count read back from the frame grid."""
    for n in range(1, c.hop + 1):
        if R.frames(c, n) >= 2:
            return np.log2(float(c.hop + 1 - n))
    raise AssertionError("early: no second frame at or below one hop")


@pytest.mark.parametrize("case", cases("cqt", "cqt_support", ("early",)))
def test_support_early(case):
    c = R.Config(**R.golden_kwargs(case["params"]))
    assert early_of(c) == case["values"][0] == float(c.early)


@pytest.mark.parametrize("case", cases("cqt", "cqt_support", ("nyquist",)))
def test_support_nyquist(case):
    try:
        R.Config(**R.golden_kwargs(case["params"]))
        accepted = 1.0
    except ValueError as e:
        accepted = 0.0
        assert "above the Nyquist frequency" in str(e)
    assert accepted == case["values"][0]


def test_the_support_file_is_whole():
    kinds = [c["params"]["kind"] for c in R.golden_cases("cqt", "cqt_support")]
    assert {k: kinds.count(k) for k in set(kinds)} == {"frequencies": 7, "filter_lengths": 8, "cutoff": 8, "early": 21, "nyquist": 3}
    assert [len(R.golden_cases("cqt", n)) for n in ("cqt_tight", "cqt_wide")] == [6, 15]


@pytest.mark.parametrize("case", cases("chroma", "chroma_fb", ("cqt_projection",)))
def test_cqt_projection_rows(case):
    """The constant-Q rows of chroma_fb.json, at 1e-12 relative (the entries are exactly zero or one)."""
    p = case["params"]
    got = R.cqt_projection(p["n_chroma"], p["bins_per_octave"], p["n_bins"], p["fmin"])
    check_close(got, case["values"], shape=case["shape"], rtol=1e-12, atol=0.0, msg=case["name"])
    assert np.array_equal(got.sum(axis=0), np.ones(p["n_bins"]))   # every bin belongs to exactly one class


@pytest.mark.parametrize("case", cases("chroma", "chroma_cqt"))
def test_chroma_cqt_goldens(case, halver):
    """chroma_goldens.ml:190-215: 1e-4 of the case peak where the plan decimates, 1e-6 at the odd hop, rtol 1e-5."""
    p = case["params"]
    c = R.Config(n_bins=p["n_bins"], sample_rate=p["sample_rate"], fmin=p["fmin"], bins_per_octave=p["bins_per_octave"],
                 tuning=p["tuning"], hop=p["hop"])
    x = R.golden_signal(p)
    if p["dtype"] == "float32":
        x = x.astype(np.float32).astype(np.float64)
    norm = {"inf": "inf", "l2": 2.0, "l1": 1.0, "none": None}[p["norm"]]
    got = R.of_cqt(c, R.power_spectrum(c, x, halver, 1.0), p["n_chroma"], norm)
    fraction = R.CHROMA_CQT_ODD_HOP_ATOL if p["hop"] % 2 == 1 else R.CHROMA_CQT_ATOL
    check_close(got, case["values"], shape=case["shape"], rtol=R.CHROMA_CQT_RTOL, atol=fraction * float(np.max(np.abs(case["values"]))),
                msg=case["name"])


def test_latency_and_frames():
    """cqt.mli:222-227: 20099 samples for the 84-bin C1 ladder at 22050 Hz and hop 512, 8192 at the odd hop (K = 190)."""
    assert R.Config(84, 22050).latency(190) == 20099
    assert R.Config(84, 22050, hop=511).latency(190) == 8192
    c = R.Config(84, 22050)
    assert [R.frames(c, n) for n in (0, 1, 100, 511, 512, 8192)] == [0, 1, 1, 1, 2, 17]
    with pytest.raises(ValueError, match="frames: cannot analyse a signal of length -1"):
        R.frames(c, -1)
