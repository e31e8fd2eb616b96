"""What of Pitch runs without a device: the flat exports and their defaults, every message word for word and in the stated order,
the frame grid, lag_range, the empty results, the stage's bookkeeping where only shapes are involved, and the agreement of the
ctypes signatures with the header."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import soundml_amd as S
from soundml_amd import Pitch, _lib, energy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")

RATE = "%s: cannot analyse audio sampled at %d Hz (sample_rate must be at least 1)"
FRAME = "%s: cannot analyse frames of %d samples (frame_length must be at least 4)"
HOP = "%s: cannot advance frames by %d samples (hop must be at least 1)"
BAND = "%s: cannot search between %s and %s Hz at %d Hz (fmin and fmax must be finite with 0 < fmin < fmax <= sample_rate / 2)"
TROUGH = "%s: cannot accept troughs below %s (trough_threshold must be finite and positive)"
SHORT = "%s: cannot search lags %d to %d in frames of %d samples (frame_length too short for fmin)"
RANK = "%s: cannot analyse a rank-zero tensor (the time axis must exist)"


def raises(message, fn, *args, **kw):
    with pytest.raises(S.InvalidArgument) as e:
        fn(*args, **kw)
    assert str(e.value) == message


def test_flat_exports_and_defaults():
    for name in ("yin", "yin_difference", "yin_stage"):
        assert getattr(S, name) is getattr(Pitch, name) and name in S.__all__ and name in S.__doc__
        p = inspect.signature(getattr(Pitch, name)).parameters
        assert p["sample_rate"].default == 22050 and p["frame_length"].default == 2048 and p["hop"].default is None
        assert p["fmin"].default is inspect.Parameter.empty and p["fmax"].default is inspect.Parameter.empty
        if name != "yin_difference":
            assert p["trough_threshold"].default == 0.1 and p["return_aperiodicity"].default is False
    assert "Pitch" in S.__all__ and Pitch.frames is energy.frames
    assert list(inspect.signature(S.yin).parameters)[:3] == ["x", "fmin", "fmax"]


def test_messages_in_the_stated_order():
    """sample_rate, frame_length, hop, the band, the threshold, the lag range, the rank: each with everything behind it wrong too"""
    x, scalar = np.zeros(100, np.float32), np.asarray(1.0, np.float32)
    for name, f in (("yin", S.yin), ("yin_difference", S.yin_difference), ("yin_stage", lambda x, *a, **k: S.yin_stage(*a, **k))):
        extra = {} if name == "yin_difference" else dict(trough_threshold=-1.0)
        raises(RATE % (name, 0), f, scalar, NAN, -1.0, sample_rate=0, frame_length=3, hop=0, **extra)
        raises(FRAME % (name, 3), f, scalar, NAN, -1.0, sample_rate=8000, frame_length=3, hop=0, **extra)
        raises(HOP % (name, 0), f, scalar, NAN, -1.0, sample_rate=8000, frame_length=64, hop=0, **extra)
        raises(HOP % (name, -2), f, scalar, 100.0, 1000.0, sample_rate=8000, frame_length=64, hop=-2)
        raises(BAND % (name, "nan", "-1", 8000), f, scalar, NAN, -1.0, sample_rate=8000, frame_length=64, **extra)
        raises(BAND % (name, "0", "1000", 8000), f, x, 0.0, 1000.0, sample_rate=8000)
        raises(BAND % (name, "1000", "1000", 8000), f, x, 1000.0, 1000.0, sample_rate=8000)
        raises(BAND % (name, "100", "4000.5", 8000), f, x, 100.0, 4000.5, sample_rate=8000)
        raises(BAND % (name, "100", "inf", 8000), f, x, 100.0, INF, sample_rate=8000)
        if extra:
            raises(TROUGH % (name, "-1"), f, scalar, 1.0, 3000.0, sample_rate=8000, frame_length=64, **extra)
            raises(TROUGH % (name, "0"), f, x, 100.0, 1000.0, sample_rate=8000, trough_threshold=0.0)
            raises(TROUGH % (name, "nan"), f, x, 100.0, 1000.0, sample_rate=8000, trough_threshold=NAN)
            raises(TROUGH % (name, "inf"), f, x, 100.0, 1000.0, sample_rate=8000, trough_threshold=INF)
        # 8000 / 4000 = 2 = the cap of a frame of 6 samples
        raises(SHORT % (name, 2, 2, 6), f, scalar, 100.0, 4000.0, sample_rate=8000, frame_length=6)
        raises(SHORT % (name, 8, 7, 16), f, scalar, 100.0, 1000.0, sample_rate=8000, frame_length=16)
        if name != "yin_stage":
            raises(RANK % name, f, scalar, 100.0, 1000.0, sample_rate=8000)
    # the default hop is a quarter of the frame
    assert S.yin(np.zeros((0, 9), np.float32), 1500.0, 4000.0, sample_rate=8000, frame_length=8).shape == (0, 1, 5)


def test_the_abi_checks_before_it_asks_for_a_device():
    lib = _lib.lib
    a = np.zeros(64, np.float32)
    ptr = C.c_void_p(a.ctypes.data)
    assert lib.smx_yin_f32(ptr, 1, 64, 0, 100.0, 1000.0, 64, 16, 0.1, ptr, None) == _lib.SMX_INVALID_ARGUMENT
    assert lib.smx_last_error().decode() == RATE % ("yin", 0)
    assert lib.smx_yin_f64(ptr, 1, 32, 8000, 100.0, 1000.0, 64, 16, -0.5, ptr, ptr) == _lib.SMX_INVALID_ARGUMENT
    assert lib.smx_last_error().decode() == TROUGH % ("yin", "-0.5")
    assert lib.smx_yin_resident_f32(ptr, 1, 64, 64, 8000, 100.0, 1000.0, 64, 0, 0.1, ptr, None, None) == _lib.SMX_INVALID_ARGUMENT
    assert lib.smx_last_error().decode() == HOP % ("yin", 0)
    assert lib.smx_yin_difference_resident_f32(ptr, 1, 64, 64, 8000, 100.0, 1000.0, 2, 1, ptr, None) == _lib.SMX_INVALID_ARGUMENT
    assert lib.smx_last_error().decode() == FRAME % ("yin_difference", 2)
    assert lib.smx_yin_frames_f32(ptr, 1, 64, 1, 8000, 1000.0, 100.0, 64, 16, 0.1, ptr, None) == _lib.SMX_INVALID_ARGUMENT
    assert lib.smx_last_error().decode() == BAND % ("yin_stage", "1000", "100", 8000)
    # a segment too short for the frames asked of it is a bookkeeping error, not the caller's
    assert lib.smx_yin_frames_f32(ptr, 1, 64, 2, 8000, 300.0, 2000.0, 64, 16, 0.1, ptr, None) == _lib.SMX_FAILURE
    assert lib.smx_yin_frames_resident_f32(ptr, 1, 63, 63, 1, 8000, 300.0, 2000.0, 64, 16, 0.1, ptr, None, None) == _lib.SMX_FAILURE
    assert lib.smx_yin_frames_f64(ptr, 1, 64, -1, 8000, 300.0, 2000.0, 64, 16, 0.1, ptr, None) == _lib.SMX_FAILURE
    # null data and zero extents: the parameters alone
    assert lib.smx_yin_f32(None, 0, 0, 8000, 300.0, 2000.0, 64, 16, 0.1, None, None) == _lib.SMX_OK
    assert lib.smx_yin_frames_f64(None, 0, 0, 0, 8000, 300.0, 2000.0, 64, 16, 0.1, None, None) == _lib.SMX_OK


def test_lag_range():
    assert Pitch.lag_range(22050, 65, 2093, 2048) == (10, 340)
    assert Pitch.lag_range(22050, 10, 2093, 2048) == (10, 1023)              # the cap: frame_length - W - 1
    assert Pitch.lag_range(8000, 100, 1000, 256) == (8, 80)
    assert Pitch.lag_range(8000, 100, 1000, 200) == (8, 80)
    assert Pitch.lag_range(8000, 300, 2000, 64) == (4, 27)
    assert Pitch.lag_range(8000, 600, 3000, 33) == (2, 14)
    assert Pitch.lag_range(8000, 600, 3000, 32) == (2, 14)
    assert Pitch.lag_range(8000, 1e-300, 3000, 33) == (2, 16)
    raises(SHORT % ("yin_difference", 8, 7, 16), Pitch.lag_range, 8000, 100.0, 1000.0, 16)
    raises(RATE % ("yin_difference", -1), Pitch.lag_range, -1, 100.0, 1000.0, 16)


def test_frame_grid_and_empty_results():
    """the grid of rms; zeros of the right shape when no signal is there at all"""
    band = dict(fmin=600.0, fmax=3000.0, sample_rate=8000)
    for fl, hop, n, count in ((32, 8, 100, 13), (33, 7, 90, 13), (32, 40, 200, 6), (2048, 512, 0, 0)):
        low = dict(band) if fl < 2048 else dict(fmin=65.0, fmax=2093.0, sample_rate=22050)
        lags = Pitch.lag_range(low["sample_rate"], low["fmin"], low["fmax"], fl)[1] + 1
        assert Pitch.frames(n, fl, hop) == count
        for dtype in (np.float32, np.float64):
            out = S.yin(np.ones((0, n), dtype), frame_length=fl, hop=hop, **low)
            assert out.shape == (0, 1, count) and out.dtype == dtype
            f0, ap = S.yin(np.ones((2, 0, n), dtype), frame_length=fl, hop=hop, return_aperiodicity=True, **low)
            assert f0.shape == ap.shape == (2, 0, 1, count) and ap.dtype == dtype
            out = S.yin_difference(np.ones((0, n), dtype), frame_length=fl, hop=hop, **low)
            assert out.shape == (0, lags, count) and out.dtype == dtype
    for dtype in (np.float32, np.float64):
        out = S.yin(np.ones((3, 0), dtype), 65.0, 2093.0)
        assert out.shape == (3, 1, 0) and out.dtype == dtype and S.yin(np.ones(0, dtype), 65, 2093).shape == (1, 0)
        assert S.yin_difference(np.ones((3, 0), dtype), 65.0, 2093.0).shape == (3, 341, 0)


def test_stage_bookkeeping_on_shapes_alone():
    """steps that complete no frame touch no device: the pending stream, the skip and the flags are host integers"""
    stage = S.yin_stage(600.0, 3000.0, sample_rate=8000, frame_length=32, hop=8)
    assert stage.latency == 16 and stage.rate == (1, 8)
    assert S.yin_stage(65, 2093).rate == (1, 512) and S.yin_stage(65, 2093).latency == 1024
    assert stage.step(np.zeros((2, 0), np.float32)) is None and not stage._started
    x = np.arange(1, 21, dtype=np.float32).reshape(2, 10)
    assert stage.step(x[:, :7]) is None                                                       # 16 border + 7 < 32
    assert stage._started and stage._pending.shape == (2, 23) and stage._pending.dtype == np.float32
    assert np.array_equal(stage._pending[:, :16], np.zeros((2, 16))) and np.array_equal(stage._pending[:, 16:], x[:, :7])
    assert stage.step(x[:, 7:]) is None and stage._pending.shape == (2, 26) and stage._skip == 0
    x[:] = 0                                                                                  # chunks are borrowed: the carry holds copies
    assert stage._pending[0, 16] == 1 and stage._tail[1, 0] == 20
    stage.reset()
    assert not stage._started and not stage._drained and stage._pending is None and stage._tail is None and stage._skip == 0
    raises("step: cannot analyse a chunk with a zero-size leading axis (channels must be at least 1)", stage.step, np.zeros((0, 5), np.float32))
    raises("step: cannot analyse a rank-zero tensor (the time axis must exist)", stage.step, np.asarray(1.0))
    assert stage.flush() == [] and stage.flush() == []
    raises("step: cannot feed a drained kernel (flush consumed the tail; reset before reusing)", stage.step, np.zeros(3, np.float32))
    # the energy stages keep their names
    assert S.rms_stage(8, 2).name == "rms_stage" and S.zero_crossing_rate_stage(8, 2).name == "zero_crossing_rate_stage"


def test_ctypes_signatures_agree_with_the_header():
    """every Pitch declaration: as many ctypes arguments as the header has parameters, in the header's order; the device forms end
    in _resident_f32, take x_stride and the stream last, and no older coverage law's pattern matches them"""
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "soundml_amd.h")).read(), flags=re.S)
    found = []
    for m in re.finditer(r"\bint (smx_yin[a-z0-9_]*)\s*\(([^)]*)\)\s*;", header):
        name, params = m.group(1), [" ".join(p.split()) for p in m.group(2).split(",")]
        want = []
        for p in params:
            if "*" in p:
                want.append(C.c_void_p)
            elif p.startswith("int64_t"):
                want.append(C.c_int64)
            elif p.startswith("double"):
                want.append(C.c_double)
            else:
                raise AssertionError("%s: unexpected parameter %r" % (name, p))
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int and args == want, name
        if "_resident" in name:
            assert name.endswith("_resident_f32") and params[-1] == "void *stream" and "int64_t x_stride" in params, name
            assert not re.search(r"smx_\w+_dev\b|smx_\w+_device_f32\b|smx_\w+_dev_f(32|64)\b", name), name
        else:
            assert name.endswith(("_f32", "_f64")) and "int64_t x_stride" not in params, name
        found.append(name)
    assert len(found) == 9 and len([n for n in found if n.endswith("_resident_f32")]) == 3, found
