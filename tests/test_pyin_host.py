"""What of pYIN runs without a device: the flat exports and their defaults, every argument error word for word and in the stated order
through the null-data calls, the pins of pyin_bins / pyin_half_width, the shapes of empty and zero-frame inputs, and the agreement of
the ctypes signatures with the header."""
import ctypes as C
import inspect
import math
import os
import re

import numpy as np
import pytest

import soundml_amd as S
from soundml_amd import Pitch, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")

RATE = "%s: cannot analyse audio sampled at %d Hz (sample_rate must be at least 1)"
FRAME = "%s: cannot analyse frames of %d samples (frame_length must be at least 4)"
HOP = "%s: cannot advance frames by %d samples (hop must be at least 1)"
BAND = "%s: cannot search between %s and %s Hz at %d Hz (fmin and fmax must be finite with 0 < fmin < fmax <= sample_rate / 2)"
SHORT = "%s: cannot search lags %d to %d in frames of %d samples (frame_length too short for fmin)"
THRESHOLDS = "%s: cannot integrate over %d thresholds (n_thresholds must be at least 1)"
BETA = "%s: cannot weigh the thresholds by a beta distribution with parameters %s and %s (beta_parameters must be finite and positive)"
BOLTZMANN = "%s: cannot weigh the troughs with a Boltzmann parameter of %s (boltzmann_parameter must be finite and positive)"
RESOLUTION = "%s: cannot resolve pitch to %s semitones (resolution must lie in (0, 1))"
MOVE = "%s: cannot let the pitch move by %s octaves per second (max_transition_rate must be finite and not negative)"
SWITCH = "%s: cannot switch voicing with probability %s (switch_prob must lie in [0, 1])"
NO_TROUGH = "%s: cannot give a frame without a trough the probability %s (no_trough_prob must lie in [0, 1])"
STATES = "%s: cannot decode %d states (2 n_bins must be at most 65535)"
CAP = "%s: cannot decode %d pitch bins with a transition half-width of %d (3 n_bins + 2 min(half_width, n_bins - 1) must be at most 9212)"
AXIS = "%s: cannot decode a state axis of %d (the state axis must be even and positive)"
WIDTH = "%s: cannot decode with a transition half-width of %d bins (half_width must not be negative)"
RANK = "%s: cannot analyse a rank-zero tensor (the time axis must exist)"


def raises(message, fn, *args, **kw):
    with pytest.raises(S.InvalidArgument) as e:
        fn(*args, **kw)
    assert str(e.value) == message


def test_flat_exports_and_defaults():
    for name in ("pyin", "pyin_observation", "pyin_decode"):
        assert getattr(S, name) is getattr(Pitch, name) and name in S.__all__ and name in S.__doc__
    for name in ("pyin", "pyin_observation", "pyin_tables"):
        p = inspect.signature(getattr(Pitch, name)).parameters
        assert p["sample_rate"].default == 22050 and p["frame_length"].default == 2048 and p["hop"].default is None
        assert p["n_thresholds"].default == 100 and p["beta_parameters"].default == (2, 18) and p["boltzmann_parameter"].default == 2.0
        assert p["resolution"].default == 0.1 and p["max_transition_rate"].default == 35.92
        assert p["switch_prob"].default == 0.01 and p["no_trough_prob"].default == 0.01
        assert p["fmin"].default is inspect.Parameter.empty and p["fmax"].default is inspect.Parameter.empty
    assert math.isnan(inspect.signature(S.pyin).parameters["fill_na"].default) and "fill_na" not in inspect.signature(S.pyin_observation).parameters
    assert list(inspect.signature(S.pyin).parameters)[:3] == ["x", "fmin", "fmax"]
    assert list(inspect.signature(S.pyin_decode).parameters) == ["obs", "half_width", "switch_prob"]
    assert inspect.signature(S.pyin_decode).parameters["switch_prob"].default == 0.01
    assert Pitch.OBSERVATION_FLOOR == 2.0 ** -200
    assert "offline" in S.pyin.__doc__.lower() and not hasattr(Pitch, "pyin_stage")


def test_messages_in_the_stated_order():
    """yin's own first, then n_thresholds, the beta parameters, the Boltzmann parameter, the resolution, the transition rate, the two
    probabilities, the state count, the decoder's cap, the rank: each with everything behind it wrong too"""
    x, scalar = np.zeros(100, np.float32), np.asarray(1.0, np.float32)
    bad = dict(n_thresholds=0, beta_parameters=(0.0, NAN), boltzmann_parameter=-1.0, resolution=1.0, max_transition_rate=-1.0, switch_prob=2.0,
               no_trough_prob=-0.5)
    for name, f in (("pyin", S.pyin), ("pyin_observation", S.pyin_observation)):
        raises(RATE % (name, 0), f, scalar, NAN, -1.0, sample_rate=0, frame_length=3, hop=0, **bad)
        raises(FRAME % (name, 3), f, scalar, NAN, -1.0, sample_rate=8000, frame_length=3, hop=0, **bad)
        raises(HOP % (name, 0), f, scalar, NAN, -1.0, sample_rate=8000, frame_length=64, hop=0, **bad)
        raises(BAND % (name, "nan", "-1", 8000), f, scalar, NAN, -1.0, sample_rate=8000, frame_length=64, **bad)
        raises(BAND % (name, "100", "4000.5", 8000), f, x, 100.0, 4000.5, sample_rate=8000)
        raises(SHORT % (name, 8, 7, 16), f, scalar, 100.0, 1000.0, sample_rate=8000, frame_length=16, **bad)
        ok = dict(sample_rate=8000, frame_length=256)
        raises(THRESHOLDS % (name, 0), f, scalar, 100.0, 1000.0, **ok, **bad)
        bad1 = dict(bad, n_thresholds=1)
        raises(BETA % (name, "0", "nan"), f, scalar, 100.0, 1000.0, **ok, **bad1)
        raises(BETA % (name, "2", "inf"), f, x, 100.0, 1000.0, beta_parameters=(2, INF), **ok)
        raises(BETA % (name, "-2", "18"), f, x, 100.0, 1000.0, beta_parameters=(-2, 18), **ok)
        bad2 = dict(bad1, beta_parameters=(0.5, 3.5))
        raises(BOLTZMANN % (name, "-1"), f, scalar, 100.0, 1000.0, **ok, **bad2)
        raises(BOLTZMANN % (name, "0"), f, x, 100.0, 1000.0, boltzmann_parameter=0.0, **ok)
        raises(BOLTZMANN % (name, "inf"), f, x, 100.0, 1000.0, boltzmann_parameter=INF, **ok)
        bad3 = dict(bad2, boltzmann_parameter=2.0)
        raises(RESOLUTION % (name, "1"), f, scalar, 100.0, 1000.0, **ok, **bad3)
        raises(RESOLUTION % (name, "0"), f, x, 100.0, 1000.0, resolution=0.0, **ok)
        raises(RESOLUTION % (name, "nan"), f, x, 100.0, 1000.0, resolution=NAN, **ok)
        bad4 = dict(bad3, resolution=0.1)
        raises(MOVE % (name, "-1"), f, scalar, 100.0, 1000.0, **ok, **bad4)
        raises(MOVE % (name, "inf"), f, x, 100.0, 1000.0, max_transition_rate=INF, **ok)
        bad5 = dict(bad4, max_transition_rate=35.92)
        raises(SWITCH % (name, "2"), f, scalar, 100.0, 1000.0, **ok, **bad5)
        raises(SWITCH % (name, "nan"), f, x, 100.0, 1000.0, switch_prob=NAN, **ok)
        bad6 = dict(bad5, switch_prob=0.0)
        raises(NO_TROUGH % (name, "-0.5"), f, scalar, 100.0, 1000.0, **ok, **bad6)
        raises(NO_TROUGH % (name, "1.5"), f, x, 100.0, 1000.0, no_trough_prob=1.5, **ok)
        # 12 * 1000 * log2(10) + 1 = 39864 bins
        raises(STATES % (name, 2 * 39864), f, scalar, 100.0, 1000.0, resolution=0.001, **ok)
        raises(RANK % name, f, scalar, 100.0, 1000.0, **ok)
        f(np.zeros((0, 10), np.float32), 100.0, 1000.0, switch_prob=1.0, no_trough_prob=1.0, max_transition_rate=0.0, **ok)
    # the decoder's cap is pyin's alone: 1994 bins with h = 1625 pass the observation
    wide = dict(sample_rate=8000, frame_length=256, resolution=0.02, max_transition_rate=104.0)
    assert Pitch.pyin_bins(100.0, 1000.0, 0.02) == 1994 and Pitch.pyin_half_width(8000, 64, 0.02, 104.0) == 250
    S.pyin(np.zeros((0, 10), np.float32), 100.0, 1000.0, **wide)
    raises(CAP % ("pyin", 1994, 1625), S.pyin, scalar, 100.0, 1000.0, **dict(wide, max_transition_rate=677.0))
    assert S.pyin_observation(np.zeros((0, 10), np.float32), 100.0, 1000.0, **dict(wide, max_transition_rate=677.0)).shape == (0, 3988, 1)


def test_decode_messages():
    name = "pyin_decode"
    obs = np.zeros((2, 8, 5), np.float32)
    raises(WIDTH % (name, -1), S.pyin_decode, np.zeros((2, 7, 5), np.float32), -1, switch_prob=3.0)
    raises(SWITCH % (name, "3"), S.pyin_decode, np.zeros((2, 7, 5), np.float32), 2, switch_prob=3.0)
    raises(SWITCH % (name, "-0.1"), S.pyin_decode, obs, 2, switch_prob=-0.1)
    lib = _lib.lib
    ptr = C.c_void_p(obs.ctypes.data)
    assert lib.smx_pyin_decode_f32(ptr, 2, 7, 5, 2, 0.01, ptr) == _lib.SMX_INVALID_ARGUMENT
    assert lib.smx_last_error().decode() == AXIS % (name, 7)
    assert lib.smx_pyin_decode_f64(ptr, 2, 0, 5, 2, 0.01, ptr) == _lib.SMX_INVALID_ARGUMENT
    assert lib.smx_last_error().decode() == AXIS % (name, 0)
    assert lib.smx_pyin_decode_accel_f32(ptr, 1, 65536, 1, 65536, 2, 0.01, ptr, None) == _lib.SMX_INVALID_ARGUMENT
    assert lib.smx_last_error().decode() == STATES % (name, 65536)
    assert lib.smx_pyin_decode_f32(ptr, 1, 9000, 1, 200, 0.01, ptr) == _lib.SMX_INVALID_ARGUMENT
    assert lib.smx_last_error().decode() == CAP % (name, 4500, 200)
    assert lib.smx_pyin_decode_f32(None, 0, 0, 0, 0, 1.0, None) == _lib.SMX_OK
    assert lib.smx_pyin_decode_accel_f32(None, 0, 0, 0, 0, 50, 0.0, None, None) == _lib.SMX_OK
    with pytest.raises(S.InvalidArgument):
        S.pyin_decode(np.zeros(8, np.float32), 2)


def test_the_abi_checks_before_it_asks_for_a_device():
    lib = _lib.lib
    a = np.zeros(64, np.float32)
    ptr = C.c_void_p(a.ctypes.data)
    good = (8000, 300.0, 2000.0, 64, 16, 100, 2.0, 18.0, 2.0, 0.1, 35.92, 0.01, 0.01)
    assert lib.smx_pyin_f32(ptr, 1, 64, *good[:5], 0, *good[6:], 0, NAN, ptr, ptr, ptr) == _lib.SMX_INVALID_ARGUMENT
    assert lib.smx_last_error().decode() == THRESHOLDS % ("pyin", 0)
    assert lib.smx_pyin_accel_f32(ptr, 1, 64, 64, *good[:9], 1.5, *good[10:], 0, NAN, ptr, ptr, ptr, None) == _lib.SMX_INVALID_ARGUMENT
    assert lib.smx_last_error().decode() == RESOLUTION % ("pyin", "1.5")
    assert lib.smx_pyin_observation_accel_f32(ptr, 1, 64, 64, 0, *good[1:], ptr, None) == _lib.SMX_INVALID_ARGUMENT
    assert lib.smx_last_error().decode() == RATE % ("pyin_observation", 0)
    assert lib.smx_pyin_observation_f64(ptr, 1, 64, *good[:12], 7.0, ptr) == _lib.SMX_INVALID_ARGUMENT
    assert lib.smx_last_error().decode() == NO_TROUGH % ("pyin_observation", "7")
    assert lib.smx_pyin_tables(*good[:7], -18.0, *good[8:], *([None] * 8)) == _lib.SMX_INVALID_ARGUMENT
    assert lib.smx_last_error().decode() == BETA % ("pyin_tables", "2", "-18")
    # null data and zero extents: the parameters alone
    assert lib.smx_pyin_f32(None, 0, 0, *good, 1, 0.0, None, None, None) == _lib.SMX_OK
    assert lib.smx_pyin_f64(None, 0, 0, *good, 0, NAN, None, None, None) == _lib.SMX_OK
    assert lib.smx_pyin_observation_f32(None, 0, 0, *good, None) == _lib.SMX_OK
    assert lib.smx_pyin_accel_f32(None, 0, 0, 0, *good, 0, NAN, None, None, None, None) == _lib.SMX_OK


def test_bins_and_half_width():
    assert Pitch.pyin_bins(65, 2093, 0.1) == 602 and Pitch.pyin_bins(65, 2093) == 602
    assert Pitch.pyin_bins(100, 1000, 0.1) == 399 and Pitch.pyin_bins(400, 500, 0.1) == 39 and Pitch.pyin_bins(100, 1000, 0.5) == 80
    assert Pitch.pyin_half_width(22050, 512, 0.1, 35.92) == 50 and Pitch.pyin_half_width() == 50
    assert Pitch.pyin_half_width(8000, 64, 0.1, 35.92) == 15 and Pitch.pyin_half_width(8000, 64, 0.5, 1.0) == 0
    assert Pitch.pyin_half_width(8000, 64, 0.1, 0.0) == 0
    # 35.92 * 12 * 512 / 22050 = 10.0087 -> 10 semitones; 2.5 and 3.5 semitones round to the even neighbour
    assert Pitch.pyin_half_width(48, 1, 0.5, 10.0) == 2 and Pitch.pyin_half_width(48, 1, 0.5, 14.0) == 4
    raises(RESOLUTION % ("pyin_bins", "1"), Pitch.pyin_bins, 65, 2093, 1.0)
    raises("pyin_bins: cannot lay bins between 100 and 50 Hz (fmin and fmax must be finite with 0 < fmin < fmax)", Pitch.pyin_bins, 100, 50, 0.1)
    raises(HOP % ("pyin_half_width", 0), Pitch.pyin_half_width, 8000, 0, 0.1, 1.0)
    raises(MOVE % ("pyin_half_width", "nan"), Pitch.pyin_half_width, 8000, 64, 0.1, NAN)
    raises("pyin_half_width: cannot let the pitch move by 1e+12 octaves per second (the band must span fewer than 2^31 bins)",
           Pitch.pyin_half_width, 8000, 64, 0.1, 1e12)


def test_empty_and_zero_frame_inputs():
    band = dict(fmin=100.0, fmax=1000.0, sample_rate=8000, frame_length=256, hop=64)
    for dtype in (np.float32, np.float64):
        for shape, lead in (((0, 900), (0,)), ((2, 0, 900), (2, 0)), ((3, 0), (3,)), ((0,), ())):
            count = Pitch.frames(shape[-1], 256, 64)
            outs = S.pyin(np.ones(shape, dtype), **band)
            assert len(outs) == 3 and all(o.shape == lead + (1, count) and o.dtype == dtype for o in outs)
            obs = S.pyin_observation(np.ones(shape, dtype), **band)
            assert obs.shape == lead + (798, count) and obs.dtype == dtype
        assert Pitch.frames(900, 256, 64) == 15 and Pitch.frames(0, 256, 64) == 0
        assert S.pyin_decode(np.ones((0, 8, 5), dtype), 2).shape == (0, 1, 5)
        assert S.pyin_decode(np.ones((4, 8, 0), dtype), 2).shape == (4, 1, 0)
        out = S.pyin_decode(np.ones((8, 0), dtype), 0)
        assert out.shape == (1, 0) and out.dtype == dtype
    with pytest.raises(S.InvalidArgument):
        S.pyin_decode(np.ones((0, 7, 5), np.float32), 2)


def test_ctypes_signatures_agree_with_the_header():
    """every pYIN declaration: as many ctypes arguments as the header has parameters, in the header's order; the device forms end in
    _accel_f32, take a stride and the stream last, and no older coverage law's pattern matches them"""
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "soundml_amd.h")).read(), flags=re.S)
    found = []
    for m in re.finditer(r"\bint (smx_pyin[a-z0-9_]*)\s*\(([^)]*)\)\s*;", header):
        name, params = m.group(1), [" ".join(p.split()) for p in m.group(2).split(",")]
        want = []
        for p in params:
            if "*" in p:
                want.append(_lib.pi64 if p.startswith("int64_t *") else C.c_void_p)
            elif p.startswith("int64_t"):
                want.append(C.c_int64)
            elif p.startswith("double"):
                want.append(C.c_double)
            else:
                raise AssertionError("%s: unexpected parameter %r" % (name, p))
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int and args == want, name
        if "_accel" in name:
            assert name.endswith("_accel_f32") and params[-1] == "void *stream", name
            assert "int64_t x_stride" in params or "int64_t clip_stride" in params, name
            taken = r"smx_\w+_dev\b|smx_\w+_device_f32\b|smx_\w+_resident_f32\b|smx_\w+_dev_f(32|64)\b|smx_\w+_gpu_f32\b|smx_\w+_hbm_f32\b|smx_\w+_vram_f32\b"
            assert not re.search(taken, name), name
        elif name.endswith(("_f32", "_f64")):
            assert "int64_t x_stride" not in params and "int64_t clip_stride" not in params, name
        found.append(name)
    assert len(found) == 12 and len([n for n in found if n.endswith("_accel_f32")]) == 3, found
