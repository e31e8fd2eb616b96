"""tempogram / tempo / beat_track on the device.

  * tempogram bit for bit against the numpy restatement (tests/rhythm_restatement.py: the one summation order of DESIGN.md 4.8g,
    where another order gives other bits, as test_rhythm_restatement.py shows) on the click tracks, each in a batch of 3 with two
    clips of noise scaled by 1e-6 and 1e6: host float32 and float64, device float32, norm on and off; the tile route against the
    general one (SMX_DISABLE_FAST=1); a leading slice; one NaN poisons exactly the frames that read it;
  * tempo_lag against the restatement's lag wherever the restatement's best score stands more than 1e-6 above the next (device
    log1p is within a few ulp of a value near 14), which the test asserts first; tempo is tempo_frequencies[lag] bit for bit;
  * beat_track's mask against the restatement's beats exactly, the library's tables and the device's lag fed in, trim on and off,
    bpm found and given; with trim the beats of a click track are its clicks.
Two NaNs count as the same bits whatever their payload."""
import contextlib
import functools
import os

import numpy as np
import pytest

import soundml_amd as S
from soundml_amd import Rhythm, Window

import rhythm_restatement as R

pytestmark = pytest.mark.gpu

GEOMETRIES = R.GEOMETRIES


@contextlib.contextmanager
def general_route():
    """SMX_DISABLE_FAST is read per call"""
    saved = os.environ.get("SMX_DISABLE_FAST")
    os.environ["SMX_DISABLE_FAST"] = "1"
    try:
        yield
    finally:
        if saved is None:
            os.environ.pop("SMX_DISABLE_FAST", None)
        else:
            os.environ["SMX_DISABLE_FAST"] = saved


def device(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()              # a copy: the cached inputs are read-only


def host(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)


def same_bits(got, want, what):
    got, want = host(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, got.dtype, want.shape, want.dtype)
    word = np.int32 if got.dtype == np.float32 else np.int64
    differ = np.ascontiguousarray(got).view(word) != np.ascontiguousarray(want).view(word)
    differ &= ~(np.isnan(got) & np.isnan(want))
    assert not differ.any(), "%s: %d/%d values differ, the first at %s: %r against %r" % (
        what, int(differ.sum()), differ.size, np.argwhere(differ)[0].tolist(), got[differ][0], want[differ][0])


def hann(W):
    return Window.make(np.float64, "hann", W)


@functools.lru_cache(maxsize=None)
def batch(geometry, dtype):
    x = R.click_batch(geometry, dtype)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def restated(geometry, dtype, norm):
    out = R.tempogram(batch(geometry, dtype), hann(geometry[2]), norm)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def restated_lags(geometry):
    """(lags, gaps) of the restatement under the library's prior"""
    frames, p, W, sr, hop = geometry
    return R.tempo_lag(batch(geometry, np.float32), hann(W), Rhythm.tempo_prior(W, sr, hop))


def faces(geometry):
    return [("host float32", batch(geometry, np.float32)), ("host float64", batch(geometry, np.float64)),
            ("device float32", device(batch(geometry, np.float32)))]


# ---- tempogram -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("norm", [True, False])
@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_tempogram_bit_for_bit_against_the_restatement(geometry, norm):
    frames, p, W = geometry[:3]
    for what, x in faces(geometry):
        want = restated(geometry, np.float64 if "64" in what else np.float32, norm)
        assert want.shape == (3, W, frames)
        same_bits(S.tempogram(x, win_length=W, norm=norm), want, what)
        with general_route():
            same_bits(S.tempogram(x, win_length=W, norm=norm), want, what + ", general route")


def test_tempogram_routes_slices_and_windows():
    for geometry in (GEOMETRIES[0], GEOMETRIES[3]):
        W = geometry[2]
        x = device(batch(geometry, np.float32))
        whole = host(S.tempogram(x, win_length=W))
        with general_route():
            same_bits(S.tempogram(x, win_length=W), whole, "the two routes")
        same_bits(S.tempogram(x[1:], win_length=W), whole[1:], "a leading slice")
        same_bits(S.tempogram(x[0], win_length=W), whole[0], "one clip")
        same_bits(S.tempogram(batch(geometry, np.float32)[:2], win_length=W), whole[:2], "a leading slice, host")
        for window in ("hamming", ("kaiser", 6.5)):
            want = R.tempogram(batch(geometry, np.float32), Window.make(np.float64, window, W))
            same_bits(S.tempogram(x, win_length=W, window=window), want, str(window))
    # a window longer than the tile route takes: the general kernel alone
    x = batch(GEOMETRIES[4], np.float32)
    same_bits(S.tempogram(device(x), win_length=600), R.tempogram(x, hann(600)), "win_length 600")


def test_tempogram_shapes():
    import torch
    x = batch(GEOMETRIES[0], np.float32)
    for xs in (x, device(x)):
        one = host(S.tempogram(xs, win_length=1))
        assert one.shape == (3, 1, 96) and np.all(one[0] == 1.0)
        same_bits(S.tempogram(xs, win_length=1, norm=False), R.tempogram(x, hann(1), False), "win_length 1")
        assert tuple(S.tempogram(xs[:, :0], win_length=8).shape) == (3, 8, 0)
        assert tuple(S.tempogram(xs[:0], win_length=8).shape) == (0, 8, 96)
        assert tuple(S.tempogram(xs.reshape(3, 1, 96)[:, :0], win_length=8).shape) == (3, 0, 8, 96)
    x64 = torch.zeros(2, 40, dtype=torch.float64, device="cuda")
    for call, op in ((lambda: S.tempogram(x64), "tempogram"), (lambda: S.tempo(x64), "tempo"), (lambda: S.beat_track(x64), "beat_track")):
        with pytest.raises(S.Failure) as e:
            call()
        assert str(e.value) == "%s: device-resident float64 envelopes are not supported; pass a host array" % op


@pytest.mark.parametrize("t0", [0, 15, 40, 95])
def test_one_nan_poisons_the_frames_that_read_it(t0):
    """frame t reads the envelope at t - 16 .. t + 15: exactly the frames t0 - 15 .. t0 + 16 are NaN (with norm at every lag, through
    a(0); without it at the lags whose chain meets the value, lag 0 among them), the rest keep the clean clip's bits"""
    geometry = GEOMETRIES[0]
    x = np.array(batch(geometry, np.float32))
    x[1, t0] = np.nan
    hit = np.zeros(96, bool)
    hit[max(0, t0 - 15):t0 + 17] = True
    for norm in (True, False):
        clean = restated(geometry, np.float32, norm)
        want = R.tempogram(x, hann(32), norm)
        for xs in (x, device(x)):
            for route in (contextlib.nullcontext(), general_route()):
                with route:
                    got = host(S.tempogram(xs, win_length=32, norm=norm))
                if norm:
                    assert np.all(np.isnan(got[1][:, hit]))
                else:                                            # lag 0 meets every value of the frame
                    assert np.all(np.isnan(got[1][0, hit]))
                assert not np.isnan(got[1][:, ~hit]).any() and not np.isnan(got[[0, 2]]).any()
                same_bits(got[1][:, ~hit], clean[1][:, ~hit], "the other frames")
                same_bits(got, want, "the whole")


# ---- tempo ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_tempo_lag_and_tempo(geometry):
    frames, p, W, sr, hop = geometry
    lags, gaps = restated_lags(geometry)
    print("restated lags", lags.tolist(), "gaps", gaps.tolist())
    assert np.all(gaps > 1e-6), gaps                             # an ambiguous input fails here
    assert lags[0] == p
    kw = dict(sample_rate=sr, hop=hop, win_length=W)
    freq = Rhythm.tempo_frequencies(W, sr, hop)
    for what, x in faces(geometry):
        dtype = host(x).dtype
        same_bits(Rhythm.tempo_lag(x, **kw), lags.astype(dtype)[:, None], what + ": lag")
        same_bits(S.tempo(x, **kw), freq[lags].astype(dtype)[:, None], what + ": tempo")
        same_bits(S.tempo(x[:2], **kw), freq[lags[:2]].astype(dtype)[:, None], what + ": a leading slice")
    with general_route():
        same_bits(Rhythm.tempo_lag(device(batch(geometry, np.float32)), **kw), lags.astype(np.float32)[:, None], "general route")


def test_tempo_of_a_nan_envelope_is_nan():
    geometry = GEOMETRIES[0]
    frames, p, W, sr, hop = geometry
    x = np.array(batch(geometry, np.float32))
    x[1, 50] = np.nan
    lags = restated_lags(geometry)[0]
    for xs in (x, device(x), x.astype(np.float64)):
        got, lag = host(S.tempo(xs, sample_rate=sr, hop=hop, win_length=W)), host(Rhythm.tempo_lag(xs, sample_rate=sr, hop=hop, win_length=W))
        assert np.isnan(got[1, 0]) and np.isnan(lag[1, 0])
        assert lag[[0, 2], 0].tolist() == lags[[0, 2]].tolist() and not np.isnan(got[[0, 2]]).any()
    assert np.isnan(host(S.tempo(device(x)[:, :0], sample_rate=sr, hop=hop, win_length=W))).all()


# ---- beat_track ----------------------------------------------------------------------------------------------------------------

def restated_masks(x, periods, trim, tightness=100.0):
    x = np.asarray(x)
    rows = []
    for c in range(x.shape[0]):
        period = int(periods[c])
        g, tx = Rhythm.beat_tables(period, tightness) if period >= 1 else (None, None)
        rows.append(R.mask_of(R.beats_of(x[c], period, g, tx, trim), x.shape[-1], x.dtype))
    return np.stack(rows)


@pytest.mark.parametrize("trim", [True, False])
@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_beat_track_against_the_restatement(geometry, trim):
    frames, p, W, sr, hop = geometry
    kw = dict(sample_rate=sr, hop=hop, win_length=W, trim=trim)
    freq = Rhythm.tempo_frequencies(W, sr, hop)
    x32 = batch(geometry, np.float32)
    # the device's own lags go into the restatement (test_tempo_lag_and_tempo compares them with the restatement's)
    lags = host(Rhythm.tempo_lag(device(x32), sample_rate=sr, hop=hop, win_length=W))[:, 0].astype(np.int64)
    want = restated_masks(x32, lags, trim)
    if trim:
        assert np.flatnonzero(want[0]).tolist() == R.clicks(frames, p).tolist()
    given = float(freq[p])
    assert Rhythm.beat_period(given, sr, hop) == p
    fixed = restated_masks(x32, [p] * 3, trim)
    for what, x in faces(geometry):
        dtype = host(x).dtype
        bpm, beats = S.beat_track(x, **kw)
        same_bits(bpm, freq[lags].astype(dtype)[:, None], what + ": tempo")
        same_bits(beats, want.astype(dtype), what + ": beats")
        assert [a.tolist() for a in Rhythm.beat_frames(beats)] == [np.flatnonzero(r).tolist() for r in want]
        bpm, beats = S.beat_track(x, bpm=given, **kw)
        same_bits(bpm, np.full((3, 1), given, dtype), what + ": the given tempo")
        same_bits(beats, fixed.astype(dtype), what + ": beats at the given tempo")
        same_bits(S.beat_track(x[1:], **kw)[1], want[1:].astype(dtype), what + ": a leading slice")


def test_beat_track_of_other_periods_and_tightness():
    """periods of more than 64 candidates (rounds of lanes), the shortest period, another tightness"""
    geometry = GEOMETRIES[1]
    frames, p, W, sr, hop = geometry
    x = batch(geometry, np.float32)
    for period, tightness in ((1, 100.0), (2, 100.0), (45, 100.0), (90, 400.0), (20, 5.0)):
        bpm = 60.0 * sr / hop / period
        assert Rhythm.beat_period(bpm, sr, hop) == period
        g, tx = Rhythm.beat_tables(period, tightness)
        want = np.stack([R.mask_of(R.beats_of(x[c], period, g, tx, True), frames, np.float32) for c in range(3)])
        for xs in (x, device(x)):
            same_bits(S.beat_track(xs, sample_rate=sr, hop=hop, bpm=bpm, tightness=tightness)[1], want, (period, tightness))


def test_clips_without_beats():
    geometry = GEOMETRIES[0]
    frames, p, W, sr, hop = geometry
    x = np.array(batch(geometry, np.float32))
    x[1] = 2.5                                                   # constant
    x[2] = 0.0                                                   # silent
    poisoned = np.array(x)
    poisoned[0, 30] = np.nan
    kw = dict(sample_rate=sr, hop=hop, win_length=W)
    clicks = R.clicks(frames, p).tolist()
    for xs in (x, device(x), x.astype(np.float64)):
        for extra in ({}, {"bpm": 120.0}):
            bpm, beats = [host(o) for o in S.beat_track(xs, **kw, **extra)]
            assert np.flatnonzero(beats[0]).tolist() == clicks and not beats[1:].any()
            if extra:
                assert np.all(bpm == 120.0)
            else:
                assert bpm[0, 0] == Rhythm.tempo_frequencies(W, sr, hop)[p]
            one = [host(o) for o in S.beat_track(xs[:, :1], **kw, **extra)]          # clips of one frame
            assert one[1].shape == (3, 1) and not one[1].any()
    for xs in (poisoned, device(poisoned)):
        bpm, beats = [host(o) for o in S.beat_track(xs, **kw)]
        assert np.isnan(bpm[0, 0]) and not beats.any()
        bpm, beats = [host(o) for o in S.beat_track(xs, bpm=120.0, **kw)]
        assert np.all(bpm == 120.0) and not beats.any()
