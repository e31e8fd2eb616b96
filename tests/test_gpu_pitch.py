"""yin / yin_difference / yin_stage on the device.

  * bit for bit against the numpy restatement (tests/pitch_restatement.py: the one summation order of DESIGN.md 4.8f) on 3 clips
    of noise scaled over 12 decades plus one tone, where another order gives other bits (test_pitch_restatement.py shows that):
    host float32 and float64, device float32;
  * the tile route against the general one (SMX_DISABLE_FAST=1), bit for bit;
  * a leading slice of a batch and a range of frames of yin_difference;
  * the partition law: every chunking of the stage, steps plus flush, is the flat call bit for bit;
  * a NaN and an Inf sample poison exactly the frames that read them.
Two NaNs count as the same bits whatever their payload."""
import contextlib
import functools
import os

import numpy as np
import pytest

import soundml_amd as S
from soundml_amd import Pitch

import pitch_restatement as R

pytestmark = pytest.mark.gpu

# (frame_length, hop, n, sample_rate, fmin, fmax): the tile route with whole blocks and 341 lags (no multiple of 64, nor of the 8
# lags of a lane); pmax at its cap 1023; the smallest tile (81 lags); a short last block; the general route: a short hop, an odd
# length, hop > frame; n < border
GEOMETRIES = [(2048, 512, 5000, 22050, 65, 2093), (2048, 512, 5000, 22050, 10, 2093), (256, 64, 1500, 8000, 100, 1000),
              (200, 64, 900, 8000, 100, 1000), (64, 16, 300, 8000, 300, 2000), (33, 7, 90, 8000, 600, 3000), (32, 40, 200, 8000, 600, 3000),
              (2048, 512, 3, 22050, 65, 2093)]
STAGE_GEOMETRIES = [(8, 2, 37, 8000, 1500, 4000), (8, 3, 37, 8000, 1500, 4000), (9, 2, 37, 8000, 1500, 4000), (64, 16, 300, 8000, 300, 2000),
                    (2048, 512, 5000, 22050, 65, 2093)]


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


def kw(geometry):
    fl, hop, n, sr, fmin, fmax = geometry
    return dict(fmin=float(fmin), fmax=float(fmax), sample_rate=sr, frame_length=fl, hop=hop)


@functools.lru_cache(maxsize=None)
def signal(geometry, dtype):
    fl, hop, n = geometry[:3]
    x = R.signals(fl * 31 + hop, n, dtype)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def restated(geometry, dtype):
    """(d', f0, aperiodicity) of the restatement, computed once"""
    fl, hop, n, sr, fmin, fmax = geometry
    x = signal(geometry, dtype)
    out = (R.yin_difference(x, fmin, fmax, sr, fl, hop),) + R.yin(x, fmin, fmax, sr, fl, hop)
    for a in out:
        a.setflags(write=False)
    return out


def check_all(x, geometry, want, what):
    fl, hop, n = geometry[:3]
    count, lags = R.frames(n, fl, hop), R.lag_range(geometry[3], geometry[4], geometry[5], fl)[1] + 1
    assert want[0].shape == (4, lags, count) and want[1].shape == (4, 1, count)
    same_bits(S.yin_difference(x, **kw(geometry)), want[0], what + " yin_difference")
    f0, ap = S.yin(x, return_aperiodicity=True, **kw(geometry))
    same_bits(f0, want[1], what + " f0")
    same_bits(ap, want[2], what + " aperiodicity")
    same_bits(S.yin(x, **kw(geometry)), want[1], what + " f0 alone")


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_bit_for_bit_against_the_restatement(geometry, dtype):
    x, want = signal(geometry, dtype), restated(geometry, dtype)
    check_all(x, geometry, want, "host")
    if dtype == np.float32:
        check_all(device(x), geometry, want, "device")
    if geometry == GEOMETRIES[0]:
        # the tone is found: its period is 1 / 0.0197 samples
        tone = want[1][3, 0, 3:-3].astype(np.float64)
        assert tone.size and np.all(np.abs(tone / (0.0197 * geometry[3]) - 1) < 3e-3)


@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_the_two_routes_give_the_same_bits(geometry):
    x, want = device(signal(geometry, np.float32)), restated(geometry, np.float32)
    with general_route():
        check_all(x, geometry, want, "general route, device")
        check_all(signal(geometry, np.float32), geometry, want, "general route, host")
    tiled = S.yin_difference(x, **kw(geometry))
    with general_route():
        same_bits(S.yin_difference(x, **kw(geometry)), host(tiled), "the two routes")


def test_a_leading_slice_and_a_frame_range():
    for geometry in (GEOMETRIES[0], GEOMETRIES[3], GEOMETRIES[4]):
        fl, hop, n = geometry[:3]
        for x in (device(signal(geometry, np.float32)), signal(geometry, np.float64)):
            whole = host(S.yin_difference(x, **kw(geometry)))
            f0, ap = S.yin(x, return_aperiodicity=True, **kw(geometry))
            same_bits(S.yin_difference(x[1:3], **kw(geometry)), whole[1:3], "a leading slice")
            same_bits(S.yin(x[2], **kw(geometry)), host(f0)[2], "one clip")
            same_bits(S.yin(x[3:], return_aperiodicity=True, **kw(geometry))[1], host(ap)[3:], "the last clip")
            # the signal from sample 3 hop on: its frame q is frame 3 + q of the whole wherever neither touches a border
            part = host(S.yin_difference(x[..., 3 * hop:], **kw(geometry)))
            inner = [q for q in range(part.shape[-1]) if q * hop - fl // 2 >= 0 and (q + 3) * hop - fl // 2 + fl <= n]
            assert len(inner) >= 2
            same_bits(part[..., inner], whole[..., [q + 3 for q in inner]], "a frame range")


def test_device_float64_is_refused():
    import torch
    x = torch.zeros(2, 100, dtype=torch.float64, device="cuda")
    band = dict(fmin=300.0, fmax=2000.0, sample_rate=8000, frame_length=64)
    for call, op in ((lambda: S.yin(x, **band), "yin"), (lambda: S.yin_difference(x, **band), "yin_difference"),
                     (lambda: S.yin_stage(**band).step(x), "yin_stage")):
        with pytest.raises(S.Failure) as e:
            call()
        assert str(e.value) == "%s: device-resident float64 audio is not supported; pass a host array" % op


# ---- the partition law -------------------------------------------------------------------------------------------------------

def chunkings(n, frame_length):
    rng = np.random.default_rng(n + frame_length)
    cuts = np.sort(rng.choice(np.arange(1, n), size=min(6, n - 1), replace=False)).tolist()
    random = [b - a for a, b in zip([0] + cuts, cuts + [n])]
    big = frame_length + 3
    out = {"one chunk": [n], "larger than the frame": [big] * (n // big) + ([n % big] if n % big else []), "random": random,
           "with empty chunks": [0, random[0], 0, 0] + random[1:] + [0]}
    if n <= 300:
        out["one sample at a time"] = [1] * n
    return out


def run_stage(stage, x, sizes):
    """the concatenation of all steps plus flush as (f0, aperiodicity)"""
    parts, at = [], 0
    for m in sizes:
        out = stage.step(x[..., at:at + m])
        at += m
        if m == 0:
            assert out is None
        if out is not None:
            assert isinstance(out, tuple) and len(out) == 2
            assert out[0].shape == out[1].shape and out[0].shape[:-1] == tuple(x.shape[:-1]) + (1,) and out[0].shape[-1] > 0
            parts.append(out)
    assert at == x.shape[-1]
    flushed = stage.flush()
    assert isinstance(flushed, list) and stage.flush() == []
    parts += flushed
    return tuple(np.concatenate([host(p[i]) for p in parts], axis=-1) for i in range(2))


@pytest.mark.parametrize("face", ["host32", "host64", "device32"])
@pytest.mark.parametrize("geometry", STAGE_GEOMETRIES)
def test_partition_law(geometry, face):
    fl, hop, n = geometry[:3]
    x = R.signals(hop, n, np.float64 if face == "host64" else np.float32)[1:]
    x = device(x) if face == "device32" else x
    flat = [host(o) for o in S.yin(x, return_aperiodicity=True, **kw(geometry))]
    assert flat[0].shape == (3, 1, R.frames(n, fl, hop))
    stage = S.yin_stage(return_aperiodicity=True, **kw(geometry))
    for name, sizes in chunkings(n, fl).items():
        stage.reset()
        got = run_stage(stage, x, sizes)
        same_bits(got[0], flat[0], name + ": f0")
        same_bits(got[1], flat[1], name + ": aperiodicity")
    single = S.yin_stage(**kw(geometry))
    out = single.step(x)
    assert not isinstance(out, tuple)
    same_bits(np.concatenate([host(out)] + [host(o) for o in single.flush()], axis=-1), flat[0], "f0 alone")


# ---- non-finite samples --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("geometry", [GEOMETRIES[2], GEOMETRIES[4]])
@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_a_non_finite_sample_poisons_the_frames_that_read_it(geometry, bad):
    """a frame reads its first W + pmax samples; those that read the sample give NaN in both outputs, every other frame the clean bits"""
    fl, hop, n, sr, fmin, fmax = geometry
    at, span = n // 2 + 1, R.used_span(fl, sr, fmin, fmax)
    x = np.array(signal(geometry, np.float32))
    x[1, at] = bad
    start = np.arange(R.frames(n, fl, hop)) * hop - fl // 2
    hit = (start <= at) & (at < start + span)
    assert 2 <= hit.sum() <= -(-span // hop)
    clean = restated(geometry, np.float32)
    want = R.yin(x, fmin, fmax, sr, fl, hop)
    for xs in (x, device(x)):
        routes = [contextlib.nullcontext(), general_route()]
        for route in routes:
            with route:
                f0, ap = [host(o) for o in S.yin(xs, return_aperiodicity=True, **kw(geometry))]
            assert np.all(np.isnan(f0[1, 0, hit])) and np.all(np.isnan(ap[1, 0, hit]))
            keep = np.ones(f0.shape, bool)
            keep[1, 0, hit] = False
            assert not np.isnan(f0[keep]).any()
            same_bits(f0[keep], clean[1][keep], "the other frames' f0")
            same_bits(ap[keep], clean[2][keep], "the other frames' aperiodicity")
            same_bits(f0, want[0], "f0")
            same_bits(ap, want[1], "aperiodicity")


def test_silence_and_a_tone_on_the_device():
    f0, ap = S.yin(device(np.zeros((2, 8192), np.float32)), 65.0, 2093.0, return_aperiodicity=True)
    assert np.all(host(f0) == np.float32(22050 / 10)) and np.all(host(ap) == 1.0)
    x = np.stack([R.harmonic_tone(t, 8192, 22050, np.float32) for t in (82.41, 440.0, 987.77)])
    f0, ap = [host(o)[:, 0, 3:-3].astype(np.float64) for o in S.yin(device(x), 65.0, 2093.0, return_aperiodicity=True)]
    assert np.all(np.abs(f0 / np.array([[82.41], [440.0], [987.77]]) - 1) <= 3e-3) and np.all(ap < 0.1)
    assert Pitch.lag_range(22050, 65, 2093) == (10, 340)
