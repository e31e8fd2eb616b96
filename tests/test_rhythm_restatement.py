"""The numpy restatement of Rhythm (tests/rhythm_restatement.py) against plain numpy formulations, and what of Rhythm runs without
a device: np.correlate for the autocorrelation, np.convolve for the local score, np.median, each to 1e-12 relative; another
summation order gives other bits; on the click tracks the chosen lag is the click period and the beats are exactly the click
frames; the library's host tables are the numpy formulas within 4 ulp; every message word for word, raised before the tensor is
looked at; the ctypes signatures agree with the header."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import soundml_amd as S
from soundml_amd import Rhythm, Window, _lib

import rhythm_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def hann(W):
    return Window.make(np.float64, "hann", W)


@functools.lru_cache(maxsize=None)
def wide(geometry):
    return R.tempogram_wide(R.click_batch(geometry), hann(geometry[2]), norm=False)


def close(got, want, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, what
    assert np.all(np.abs(got - want) <= 1e-12 * np.max(np.abs(want))), what


@pytest.mark.parametrize("geometry", R.GEOMETRIES[:5])
def test_autocorrelation_against_correlate(geometry):
    frames, p, W = geometry[:3]
    x = R.click_batch(geometry)
    y = R.frames_of(x, hann(W))
    a = wide(geometry)
    assert a.shape == (3, frames, W)
    for c in range(3):
        for t in range(frames):
            close(a[c, t], np.correlate(y[c, t], y[c, t], "full")[W - 1:], (c, t))
    # the normalised form: lag 0 is exactly 1 wherever the frame has energy
    n = R.tempogram_wide(x, hann(W), norm=True)
    assert np.all(n[..., 0] == 1.0)
    assert R.tempogram(x, hann(W)).shape == (3, W, frames) and R.tempogram(x, hann(W)).dtype == np.float32


def test_another_order_gives_other_bits():
    geometry = R.GEOMETRIES[0]
    y = R.frames_of(R.click_batch(geometry), hann(geometry[2]))
    up, down = R.autocorrelation(y), R.autocorrelation(y, descending=True)
    close(up, down, "the two orders agree to rounding")
    assert (up != down).mean() > 0.05


def test_zeros_and_the_virtual_border():
    """a silent clip stays zero under norm (0 < DBL_MIN: left as it is); the first frame sees W - W // 2 values of the clip"""
    assert np.all(R.tempogram(np.zeros((1, 9), np.float32), hann(4)) == 0)
    x = np.arange(1, 7, dtype=np.float64)[None]
    w = np.ones(5)
    a = R.tempogram_wide(x, w, norm=False)
    assert a[0, 0, 0] == 1 + 4 + 9 and a[0, 0, 1] == 1 * 2 + 2 * 3 and a[0, 5, 0] == 16 + 25 + 36


@pytest.mark.parametrize("geometry", R.GEOMETRIES)
def test_click_tracks_have_their_lag_and_their_beats(geometry):
    frames, p, W, sr, hop = geometry
    x = R.click_batch(geometry)
    prior = Rhythm.tempo_prior(W, sr, hop)
    lags, gaps = R.tempo_lag(x, hann(W), prior)
    assert lags[0] == p and np.all(gaps > 1e-6), (lags, gaps)
    assert Rhythm.tempo_frequencies(W, sr, hop)[p] == 60.0 * sr / (hop * p)
    g, tx = Rhythm.beat_tables(p)
    want = R.clicks(frames, p).tolist()
    assert R.beats_of(x[0], p, g, tx, True).tolist() == want
    # untrimmed, the walk may start behind the last click (cum still rises where the last frame lies more than half a period
    # behind it: (200, 20) ends on 199) and may end before the first (the 7-frame clip: 0): what trimming is there to drop
    loose = R.beats_of(x[0], p, g, tx, False).tolist()
    assert [i for i in loose if want[0] <= i <= want[-1]] == want and len(loose) <= len(want) + 2


def test_local_score_and_median_against_numpy():
    rng = np.random.default_rng(5)
    for frames, p in ((50, 4), (9, 7), (200, 20), (3, 5)):
        ne = rng.standard_normal(frames)
        g, _ = Rhythm.beat_tables(p)
        close(R.local_score(ne, g, p), np.convolve(ne, g, "full")[p:p + frames], (frames, p))
    for n in (1, 2, 7, 10):
        v = rng.standard_normal(n)
        assert R.median(v) == np.median(v)
    v = rng.standard_normal(40)
    assert R.deviation(v) == pytest.approx(np.std(v, ddof=1), rel=1e-12)


def test_no_beats():
    g, tx = Rhythm.beat_tables(4)
    x = R.click_batch(R.GEOMETRIES[0])[0]
    for env in (np.full(30, 2.5), np.zeros(30), x[:1], np.where(np.arange(96) == 40, np.nan, x)):
        assert R.beats_of(env, 4, g, tx).size == 0
    assert R.beats_of(x, 0, g, tx).size == 0


def ulps(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    same = (got == want) | (np.isnan(got) & np.isnan(want))
    with np.errstate(all="ignore"):
        return np.where(same, 0.0, np.abs(got - want) / np.spacing(np.abs(want)))


def test_tables_are_the_numpy_formulas_within_4_ulp():
    for p in (1, 2, 5, 8, 21, 64, 383):
        g, tx = Rhythm.beat_tables(p, 100.0)
        window = np.arange(-2 * p, -R.half_even(p) + 1)
        assert len(g) == 2 * p + 1 and len(tx) == len(window) and R.half_even(p) == int(np.round(p / 2))
        with np.errstate(all="ignore"):
            assert ulps(g, np.exp(-0.5 * (np.arange(-p, p + 1) * 32.0 / p) ** 2)).max() <= 4
            assert ulps(tx, -100.0 * np.log(-window / p) ** 2).max() <= 4
    for W, sr, hop in ((384, 22050, 512), (32, 8000, 500), (8, 8000, 1000)):
        with np.errstate(all="ignore"):
            bpm = 60.0 * sr / (hop * np.arange(W, dtype=np.float64))
            want = np.where((np.arange(W) == 0) | (bpm > 320.0), -np.inf, -0.5 * ((np.log2(bpm) - np.log2(120.0)) / 1.0) ** 2)
        assert np.array_equal(Rhythm.tempo_frequencies(W, sr, hop), bpm)
        assert ulps(Rhythm.tempo_prior(W, sr, hop), want).max() <= 4
    assert Rhythm.beat_period(120.0, 22050, 512) == 22 and Rhythm.beat_period(100.0, 8000, 500) == 10     # 9.6 -> 10
    assert Rhythm.beat_period(60.0 * 16 / 2.5, 8000, 500) == 2 and Rhythm.beat_period(60.0 * 16 / 3.5, 8000, 500) == 4   # halves go to even


# ---- messages, before the tensor is looked at ----------------------------------------------------------------------------------

def raises(message, fn, *args, **kw):
    with pytest.raises(S.InvalidArgument) as e:
        fn(*args, **kw)
    assert str(e.value) == message


def test_flat_exports():
    for name in ("tempogram", "tempo", "beat_track"):
        assert getattr(S, name) is getattr(Rhythm, name) and name in S.__all__ and name in S.__doc__
    assert "Rhythm" in S.__all__


def test_messages():
    scalar = np.asarray(1.0, np.float32)                        # a rank-zero tensor: every parameter error comes first
    WIN = "%s: cannot correlate windows of %d frames (win_length must lie in [1, 16384])"
    HOP = "%s: cannot advance frames by %d samples (hop must be at least 1)"
    raises(WIN % ("tempogram", 0), S.tempogram, scalar, win_length=0)
    raises(WIN % ("tempo", -3), S.tempo, scalar, win_length=-3)
    raises(WIN % ("beat_track", 0), S.beat_track, scalar, win_length=0)
    raises("tempogram: unknown window family 'bogus'", S.tempogram, scalar, window="bogus")
    raises(HOP % ("tempo", 0), S.tempo, scalar, hop=0)
    raises(HOP % ("beat_track", -1), S.beat_track, scalar, hop=-1, bpm=-1.0)
    raises("tempo: cannot analyse audio sampled at 0 Hz (sample_rate must be at least 1)", S.tempo, scalar, sample_rate=0, hop=0)
    raises("beat_track: cannot track beats at 0 beats per minute (bpm must be finite and positive)", S.beat_track, scalar, bpm=0.0)
    raises("beat_track: cannot track beats at -2 beats per minute (bpm must be finite and positive)", S.beat_track, scalar, bpm=-2.0, tightness=0.0)
    raises("beat_track: a beat at 1e+06 beats per minute lasts 0 frames (the period must lie in [1, 4096])", S.beat_track, scalar, bpm=1e6)
    raises("tempo: cannot use a prior 0 octaves wide (std_bpm must be finite and positive)", S.tempo, scalar, std_bpm=0.0)
    raises("tempo: cannot use a prior -1 octaves wide (std_bpm must be finite and positive)", S.tempo, scalar, std_bpm=-1.0, max_tempo=-1.0)
    raises("tempo: cannot centre the prior at 0 beats per minute (start_bpm must be finite and positive)", S.tempo, scalar, start_bpm=0.0)
    raises("beat_track: cannot weigh the tempo by 0 (tightness must be finite and positive)", S.beat_track, scalar, tightness=0.0)
    raises("beat_track: cannot weigh the tempo by -5 (tightness must be finite and positive)", S.beat_track, scalar, bpm=120.0, tightness=-5.0)
    # 60 * 22050 / (512 * 7) = 369 bpm: no lag of an 8-frame window is slow enough
    NONE = "%s: no lag of a %d-frame window is at or below %s beats per minute (win_length too short for max_tempo)"
    raises(NONE % ("tempo", 8, "320"), S.tempo, scalar, win_length=8)
    raises(NONE % ("tempo", 1, "320"), S.tempo, scalar, win_length=1)
    raises(NONE % ("beat_track", 8, "320"), S.beat_track, scalar, win_length=8)
    raises(NONE % ("tempo", 384, "5"), Rhythm.tempo_lag, scalar, max_tempo=5.0)
    raises("beat_track: cannot track a clip of 8193 frames (at most 8192)", S.beat_track, np.zeros(8193, np.float32), bpm=120.0)
    raises("tempo: cannot analyse a rank-zero tensor (the time axis must exist)", S.tempo, scalar)


def test_shapes_without_a_device():
    for dtype in (np.float32, np.float64):
        assert S.tempogram(np.ones((0, 5), dtype), win_length=1).shape == (0, 1, 5)
        out = S.tempogram(np.ones((2, 0), dtype), win_length=7)
        assert out.shape == (2, 7, 0) and out.dtype == dtype
        assert S.tempogram(np.ones((3, 0, 9), dtype)).shape == (3, 0, 384, 9)
        assert S.tempo(np.ones((0, 5), dtype)).shape == (0, 1) and S.tempo(np.ones((0, 5), dtype)).dtype == dtype
        bpm, beats = S.beat_track(np.ones((0, 5), dtype))
        assert bpm.shape == (0, 1) and beats.shape == (0, 5) and beats.dtype == dtype
        # no frames: the tempo of nothing is NaN, a given bpm is reported as it is
        assert np.isnan(S.tempo(np.ones((2, 0), dtype))).all()
        bpm, beats = S.beat_track(np.ones((2, 0), dtype), bpm=90.0)
        assert np.all(bpm == 90.0) and beats.shape == (2, 0)
    masks = np.array([[0, 1, 0, 1], [1, 0, 0, 0]], np.float32)
    assert [a.tolist() for a in Rhythm.beat_frames(masks)] == [[1, 3], [0]] and Rhythm.beat_frames(masks[0]).tolist() == [1, 3]


def test_ctypes_signatures_agree_with_the_header():
    """every Rhythm declaration: as many ctypes arguments as the header has parameters, in the header's order; the device forms end
    in _gpu_f32, take env_stride and the stream last, and no older coverage law's pattern matches them"""
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "soundml_amd.h")).read(), flags=re.S)
    kinds = {"int64_t": C.c_int64, "double": C.c_double, "int": C.c_int}
    found = []
    for m in re.finditer(r"\bint (smx_rhythm[a-z0-9_]*)\s*\(([^)]*)\)\s*;", header):
        name, params = m.group(1), [" ".join(p.split()) for p in m.group(2).split(",")]
        want = []
        for p in params:
            if p == "int64_t *period":
                want.append(C.POINTER(C.c_int64))
            elif "*" in p:
                want.append(C.c_void_p)
            else:
                want.append(kinds[p.split(" ")[0]])
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int and args == want, name
        if "_gpu_" in name:
            assert name.endswith("_gpu_f32") and params[-1] == "void *stream" and "int64_t env_stride" in params, name
            assert not re.search(r"smx_\w+_dev\b|smx_\w+_device_f32\b|smx_\w+_dev_f(32|64)\b|smx_\w+_resident_f32\b", name), name
        found.append(name)
    assert len(found) == 13 and len([n for n in found if n.endswith("_gpu_f32")]) == 3, found
