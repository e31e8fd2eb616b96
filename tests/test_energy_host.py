"""What of the energy features runs without a device: the flat re-exports and their defaults, every Invalid_argument of energy.ml
word for word and in the reference's order, the frame grid, the empty results, the stages' bookkeeping where only shapes are
involved, and the agreement of the ctypes signatures with the header."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import soundml_amd as S
from soundml_amd import _lib, energy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = float("nan"), float("inf")

THRESHOLD = "%s: cannot clamp signs with a threshold of %s (threshold must be finite and non-negative)"
FRAME = "%s: cannot analyse frames of %d samples (frame_length must be at least 1)"
HOP = "%s: cannot advance frames by %d samples (hop must be at least 1)"
RANK = "%s: cannot analyse a rank-zero tensor (the time axis must exist)"


def raises(message, fn, *args, **kw):
    with pytest.raises(S.InvalidArgument) as e:
        fn(*args, **kw)
    assert str(e.value) == message


def test_flat_reexports_and_defaults():
    for name in ("rms", "rms_of_spectrogram", "rms_stage", "zero_crossing_rate", "zero_crossing_rate_stage"):
        assert getattr(S, name) is getattr(energy, name) and name in S.__all__ and name in S.__doc__
        p = inspect.signature(getattr(energy, name)).parameters
        assert p["frame_length"].default == 2048
        if name != "rms_of_spectrogram":
            assert p["hop"].default == 512
        assert ("threshold" in p) == name.startswith("zero")
        if "threshold" in p:
            assert p["threshold"].default == 1e-10


def test_flat_messages_in_the_reference_order():
    """energy.ml:360-388: the threshold, the frame length, the hop, the rank"""
    x, scalar = np.zeros(100, np.float32), np.asarray(1.0, np.float32)
    z = "zero_crossing_rate"
    raises(THRESHOLD % (z, "-1"), S.zero_crossing_rate, scalar, frame_length=0, hop=0, threshold=-1.0)
    raises(THRESHOLD % (z, "nan"), S.zero_crossing_rate, x, threshold=NAN)
    raises(THRESHOLD % (z, "inf"), S.zero_crossing_rate, x, threshold=INF)
    raises(THRESHOLD % (z, "-1e-300"), S.zero_crossing_rate, x, threshold=-1e-300)
    raises(FRAME % (z, 0), S.zero_crossing_rate, scalar, frame_length=0, hop=0)
    raises(HOP % (z, 0), S.zero_crossing_rate, scalar, frame_length=1, hop=0)
    raises(RANK % z, S.zero_crossing_rate, scalar)
    raises(FRAME % ("rms", 0), S.rms, scalar, frame_length=0, hop=0)
    raises(FRAME % ("rms", -5), S.rms, x, frame_length=-5)
    raises(HOP % ("rms", -2), S.rms, scalar, hop=-2)
    raises(RANK % "rms", S.rms, scalar)


def test_stage_messages_in_the_reference_order():
    """energy.ml:514-525: the frame length, the hop, then the threshold; energy.ml:290-298 for the steps"""
    z = "zero_crossing_rate_stage"
    raises(FRAME % (z, 0), S.zero_crossing_rate_stage, 0, 0, -1.0)
    raises(HOP % (z, 0), S.zero_crossing_rate_stage, 4, 0, -1.0)
    raises(THRESHOLD % (z, "-1"), S.zero_crossing_rate_stage, 4, 2, -1.0)
    raises(FRAME % ("rms_stage", 0), S.rms_stage, 0, 0)
    raises(HOP % ("rms_stage", 0), S.rms_stage, 4, 0)
    for stage in (S.rms_stage(8, 2), S.zero_crossing_rate_stage(8, 2)):
        raises("step: cannot analyse a chunk with a zero-size leading axis (channels must be at least 1)", stage.step, np.zeros((0, 5), np.float32))
        raises("step: cannot analyse a chunk with a zero-size leading axis (channels must be at least 1)", stage.step, np.zeros((2, 0, 0)))
        assert stage.flush() == [] and stage.flush() == []
        raises("step: cannot feed a drained kernel (flush consumed the tail; reset before reusing)", stage.step, np.zeros(3, np.float32))
        raises("step: cannot feed a drained kernel (flush consumed the tail; reset before reusing)", stage.step, np.zeros((0, 5)))


def test_rms_of_spectrogram_messages_in_the_reference_order():
    """energy.ml:394-408: the frame length, the rank, the bin count"""
    op = "rms_of_spectrogram"
    raises(FRAME % (op, 0), S.rms_of_spectrogram, np.zeros(5, np.float32), frame_length=0)
    raises("%s: cannot analyse a rank-1 tensor (the spectrogram path needs [...; bins; frames])" % op, S.rms_of_spectrogram, np.zeros(5), 16)
    raises("%s: cannot analyse a rank-0 tensor (the spectrogram path needs [...; bins; frames])" % op, S.rms_of_spectrogram, np.asarray(1.0))
    bins = "%s: cannot read %d frequency bins as frames of %d samples (a magnitude spectrogram holds frame_length / 2 + 1 bins)"
    raises(bins % (op, 8, 16), S.rms_of_spectrogram, np.zeros((8, 3), np.float32), 16)
    raises(bins % (op, 9, 15), S.rms_of_spectrogram, np.zeros((0, 9, 3)), frame_length=15)
    raises(bins % (op, 1024, 2048), S.rms_of_spectrogram, np.zeros((1024, 0)))


def test_the_abi_checks_before_it_asks_for_a_device():
    lib = _lib.lib
    a = np.zeros(64, np.float32)
    ptr = C.c_void_p(a.ctypes.data)
    assert lib.smx_rms_f32(ptr, 1, 64, 0, 4, ptr) == _lib.SMX_INVALID_ARGUMENT
    assert lib.smx_last_error().decode() == FRAME % ("rms", 0)
    assert lib.smx_zero_crossing_rate_f64(ptr, 1, 32, 0, 0, -2.0, ptr) == _lib.SMX_INVALID_ARGUMENT
    assert lib.smx_last_error().decode() == THRESHOLD % ("zero_crossing_rate", "-2")
    assert lib.smx_rms_device_f32(ptr, 1, 64, 64, 8, 0, ptr, None) == _lib.SMX_INVALID_ARGUMENT
    assert lib.smx_last_error().decode() == HOP % ("rms", 0)
    assert lib.smx_rms_of_spectrogram_f32(ptr, 1, 8, 8, 16, ptr) == _lib.SMX_INVALID_ARGUMENT
    assert lib.smx_energy_frames_f32(1, NAN, 8, 2, ptr, 1, 64, 3, ptr) == _lib.SMX_INVALID_ARGUMENT
    assert lib.smx_last_error().decode() == THRESHOLD % ("zero_crossing_rate_stage", "nan")
    # a segment too short for the frames asked of it is a bookkeeping error, not the caller's
    assert lib.smx_energy_frames_f32(0, 0.0, 8, 2, ptr, 1, 11, 3, ptr) == _lib.SMX_FAILURE
    assert lib.smx_energy_frames_device_f32(0, 0.0, 8, 2, ptr, 1, 7, 7, 1, ptr, None) == _lib.SMX_FAILURE
    assert lib.smx_energy_frames_f32(2, 0.0, 8, 2, None, 0, 0, 0, None) == _lib.SMX_FAILURE


def test_frame_grid_and_empty_results():
    """energy.ml:114-118, 354-366: no frames for an empty signal; zeros of [...; 1; count] when no signal is there at all"""
    for fl, hop, n, count in ((16, 4, 100, 26), (15, 7, 64, 10), (8, 11, 60, 6), (1, 3, 20, 7), (2048, 512, 0, 0), (2048, 512, 1, 1)):
        assert energy.frames(n, fl, hop) == count
        for dtype in (np.float32, np.float64):
            for f in (S.rms, S.zero_crossing_rate):
                out = f(np.ones((0, n), dtype), fl, hop)
                assert out.shape == (0, 1, count) and out.dtype == dtype
                out = f(np.ones((2, 0, n), dtype), frame_length=fl, hop=hop)
                assert out.shape == (2, 0, 1, count)
    for dtype in (np.float32, np.float64):
        for f in (S.rms, S.zero_crossing_rate):
            out = f(np.ones((3, 0), dtype))
            assert out.shape == (3, 1, 0) and out.dtype == dtype
            assert f(np.ones(0, dtype), 8, 3).shape == (1, 0)
        assert S.rms_of_spectrogram(np.ones((0, 9, 5), dtype), 16).shape == (0, 1, 5)
        out = S.rms_of_spectrogram(np.ones((2, 9, 0), dtype), 16)
        assert out.shape == (2, 1, 0) and out.dtype == dtype


def test_stage_bookkeeping_on_shapes_alone():
    """steps that complete no frame touch no device: the pending stream, the skip and the flags are host integers"""
    for make in (S.rms_stage, S.zero_crossing_rate_stage):
        stage = make(frame_length=8, hop=2)
        assert stage.latency == 4 and stage.rate == (1, 2)
        assert stage.step(np.zeros((2, 0), np.float32)) is None and not stage._started          # an empty chunk changes nothing
        x = np.arange(1, 7, dtype=np.float32).reshape(2, 3)
        assert stage.step(x[:, :2]) is None                                                       # 4 border + 2 < 8
        assert stage._started and stage._pending.shape == (2, 6) and stage._pending.dtype == np.float32
        edge = make is S.zero_crossing_rate_stage
        assert np.array_equal(stage._pending[:, :4], np.repeat(x[:, :1], 4, axis=1) if edge else np.zeros((2, 4)))
        assert np.array_equal(stage._tail, x[:, 1:2])
        assert stage.step(x[:, 2:]) is None and stage._pending.shape == (2, 7)
        assert np.array_equal(stage._tail, x[:, 2:]) and stage._skip == 0
        x[:] = 0                                                                                  # chunks are borrowed: the carry holds copies
        assert stage._pending[0, 4] == 1 and stage._tail[1, 0] == 6
        stage.reset()
        assert not stage._started and not stage._drained and stage._pending is None and stage._tail is None and stage._skip == 0
    stage = S.rms_stage(frame_length=1, hop=3)
    assert stage.latency == 0 and stage.flush() == []
    with pytest.raises(S.InvalidArgument):
        stage.step(np.asarray(1.0))


def test_ctypes_signatures_agree_with_the_header():
    """every energy declaration: as many ctypes arguments as the header has parameters, in the header's order; the device forms
    end in _device_f32 and take the stream last"""
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "soundml_amd.h")).read(), flags=re.S)
    found = []
    for m in re.finditer(r"\bint (smx_(?:rms|zero_crossing_rate|energy_frames)[a-z0-9_]*)\s*\(([^)]*)\)\s*;", header):
        name, params = m.group(1), [p.strip() for p in m.group(2).split(",")]
        want = []
        for p in params:
            if "*" in p:
                want.append(C.c_void_p)
            elif p.startswith("int64_t"):
                want.append(C.c_int64)
            elif p.startswith("double"):
                want.append(C.c_double)
            elif p.startswith("int "):
                want.append(C.c_int)
            else:
                raise AssertionError("%s: unexpected parameter %r" % (name, p))
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int and args == want, name
        if "_device" in name:
            assert name.endswith("_device_f32") and params[-1] == "void *stream", name
            assert ("int64_t x_stride" in params) == ("spectrogram" not in name), name      # audio rows may be pitched
        else:
            assert name.endswith(("_f32", "_f64")), name
        found.append(name)
    assert len(found) == 12 and len([n for n in found if n.endswith("_device_f32")]) == 4, found
