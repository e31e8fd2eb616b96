"""What of Effects runs without a device: ``semitones``, the output lengths, the argument checks (effects.ml:96-123,
316-322, 349-383, in the reference's order and words, before any device work), the empty results, and the agreement of the
ctypes signatures with the header."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import soundml_amd as S
from soundml_amd import Effects, Stft, _lib

import effects_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FACES = ["phase_vocoder", "time_stretch", "pitch_shift", "semitones"]


def config(fft_size=64, hop=16):
    return Stft.Config.create(fft_size=fft_size, hop=hop)


# ---- semitones ------------------------------------------------------------------------------------------------------
def test_semitones_documented_values():
    assert Effects.semitones(12) == (2, 1)
    assert Effects.semitones(-12) == (1, 2)
    assert Effects.semitones(4) == (349, 277)
    assert Effects.semitones(0) == (1, 1) and Effects.semitones(24) == (4, 1) and Effects.semitones(-24) == (1, 4)
    assert Effects.semitones(108) == (512, 1) and Effects.semitones(-108) == (1, 512)   # nine octaves: the last ratio inside the cap


def test_semitones_against_the_restatement():
    for quarter in range(-96, 97):
        n = quarter / 4.0
        assert Effects.semitones(n) == R.semitones(n), n
    for bins_per_octave in (24, 19):
        for n in range(-2 * bins_per_octave, 2 * bins_per_octave + 1):
            assert Effects.semitones(n, bins_per_octave) == R.semitones(n, bins_per_octave), (n, bins_per_octave)
            assert Effects.semitones(n + 0.5, bins_per_octave=bins_per_octave) == R.semitones(n + 0.5, bins_per_octave)


def test_semitones_lands_within_the_documented_cents():
    for steps in range(-12, 13):   # effects.mli:246-248
        num, den = Effects.semitones(steps)
        assert abs(1200.0 * np.log2(num / den) - 100.0 * steps) <= 0.027


NAN, INF = float("nan"), float("inf")


@pytest.mark.parametrize("n, bins_per_octave, message", [
    (4.0, 0, "semitones: cannot divide the octave into 0 steps (bins_per_octave must be at least 1)"),
    (NAN, -3, "semitones: cannot divide the octave into -3 steps (bins_per_octave must be at least 1)"),   # the resolution first
    (NAN, 12, "semitones: cannot shift by nan steps (the step count must be finite)"),
    (INF, 12, "semitones: cannot shift by inf steps (the step count must be finite)"),
    (-INF, 12, "semitones: cannot shift by -inf steps (the step count must be finite)"),
    (156.0, 12, "semitones: cannot represent a frequency ratio of 8192 within 512 (the step count is too far from unity)"),
    (120.0, 12, "semitones: cannot represent a frequency ratio of 1024 within 512 (the step count is too far from unity)"),
    (-120.0, 12, "semitones: cannot represent a frequency ratio of 0.000976562 within 512 (the step count is too far from unity)"),
])
def test_semitones_messages(n, bins_per_octave, message):
    with pytest.raises(S.InvalidArgument) as e:
        Effects.semitones(n, bins_per_octave=bins_per_octave)
    assert str(e.value) == message
    with pytest.raises(ValueError) as r:   # the restatement words them the same way
        R.semitones(n, bins_per_octave)
    assert str(r.value) == message


def test_semitones_beyond_nine_octaves():
    """Upwards nothing is representable past 512/1; downwards 1/512 stays the nearest admissible ratio until the rounded
    numerator reaches 0, a further octave down: the reference's search, which the restatement repeats."""
    for n in (108.25, 109, 131.5, 1000.0, -120.25, -121, -1000.0):
        with pytest.raises(S.InvalidArgument):
            Effects.semitones(n)
        with pytest.raises(ValueError):
            R.semitones(n)
    for n in (-108.25, -109, -119.75):
        assert Effects.semitones(n) == R.semitones(n) == (1, 512)


# ---- lengths --------------------------------------------------------------------------------------------------------
def test_time_stretch_length_rounds_ties_to_even():
    assert Effects.stretch_length(5, 2.0) == 2 and Effects.stretch_length(7, 2.0) == 4
    assert Effects.stretch_length(1, 2.0) == 0 and Effects.stretch_length(3, 2.0) == 2
    for n in (0, 1, 127, 1000, 20000):
        for rate in (0.5, 0.75, 1.0, 1.37, 2.0, 3.7, 1.0 / 3.0):
            assert Effects.stretch_length(n, rate) == R.stretch_length(n, rate)


def test_phase_vocoder_frames():
    assert Effects.out_frames(0, 0.5) == 0 and Effects.out_frames(9, 2.0) == 5 and Effects.out_frames(9, 0.75) == 12
    for frames in (0, 1, 9, 26, 37, 130):
        for rate in (0.5, 0.75, 1.0, 1.25, 1.37, 2.0, 3.7, 1.0 / 3.0):
            assert Effects.out_frames(frames, rate) == R.out_frames(frames, rate)


# ---- validation -----------------------------------------------------------------------------------------------------
RATES = [(0.0, "0"), (-1.5, "-1.5"), (float("nan"), "nan"), (float("inf"), "inf"), (float("-inf"), "-inf")]


@pytest.mark.parametrize("rate, text", RATES)
def test_rate_messages_come_first(rate, text):
    c = config()
    # the rate is checked before the rank and the bin axis (effects.ml:285-287, 291-293)
    for fn, arg in (("phase_vocoder", np.zeros(5, np.complex64)), ("phase_vocoder", np.zeros((7, 4), np.complex128)),
                    ("time_stretch", np.asarray(1.0, np.float32)), ("time_stretch", np.zeros(100, np.float64))):
        with pytest.raises(S.InvalidArgument) as e:
            getattr(Effects, fn)(c, arg, rate)
        assert str(e.value) == "%s: cannot stretch by a rate of %s (the rate must be finite and positive)" % (fn, text)


def test_spectrum_messages():
    c = config()
    with pytest.raises(S.InvalidArgument) as e:
        Effects.phase_vocoder(c, np.zeros(33, np.complex64), 1.5)
    assert str(e.value) == "phase_vocoder: cannot vocode a rank-1 tensor (the bin and frame axes must exist)"
    with pytest.raises(S.InvalidArgument) as e:
        Effects.phase_vocoder(c, np.asarray(1j, np.complex128), 1.5)
    assert str(e.value) == "phase_vocoder: cannot vocode a rank-0 tensor (the bin and frame axes must exist)"
    with pytest.raises(S.InvalidArgument) as e:
        Effects.phase_vocoder(c, np.zeros((2, 32, 9), np.complex64), 1.5)
    assert str(e.value) == ("phase_vocoder: cannot vocode 32 frequency bins of a 64-point transform (the bin axis must hold "
                            "fft_size / 2 + 1 = 33 values)")


def test_signal_messages():
    c = config()
    for fn, arg in (("time_stretch", 1.5), ("pitch_shift", (3, 2))):
        with pytest.raises(S.InvalidArgument) as e:
            getattr(Effects, fn)(c, np.asarray(1.0, np.float64), arg)
        assert str(e.value) == "%s: cannot process a rank-zero tensor (the time axis must exist)" % fn
    for ratio in ((0, 2), (3, -2), (-1, -1)):   # the ratio comes before the rank (effects.ml:326-327)
        with pytest.raises(S.InvalidArgument) as e:
            Effects.pitch_shift(c, np.asarray(1.0, np.float32), ratio)
        assert str(e.value) == "pitch_shift: cannot shift by a frequency ratio of %d/%d (both terms must be at least 1)" % ratio
    for fn, arg in (("phase_vocoder", np.zeros((33, 4), np.complex64)), ("time_stretch", np.zeros(100, np.float32))):
        with pytest.raises(S.InvalidArgument) as e:
            getattr(Effects, fn)(c, arg, 1.5, phase="loose")
        assert str(e.value).startswith("%s: cannot use phase 'loose'" % fn)


def test_conditions_of_invert_and_of_the_resampler_raise_from_where_they_do():
    # a periodic Hann advanced by its own length overlap-adds to zero at the frame boundary (pvoc_edge.ml:351-360)
    gaps = Stft.Config.create(fft_size=64, hop=64)
    assert not Stft.nola(gaps)
    x = np.zeros(1000, np.float32)
    for call in (lambda: Effects.time_stretch(gaps, x, 1.5), lambda: Effects.pitch_shift(gaps, x, (3, 2)),
                 lambda: Effects.pitch_shift(gaps, x, (3524, 2797), quality="best")):   # (the stretch's conditions come first)
        with pytest.raises(S.InvalidArgument) as e:
            call()
        assert str(e.value).startswith("invert: cannot invert a 64-point window advanced by 64 samples")
    with pytest.raises(S.InvalidArgument) as e:
        Effects.pitch_shift(config(), x, (100003, 100019))
    assert str(e.value).startswith("create: cannot resample 100003 Hz to 100019 Hz")


def test_the_abi_checks_before_it_asks_for_a_device():
    """The C entry points word the same errors themselves, before require_device: SMX_INVALID_ARGUMENT, not the
    missing-device Failure, whether or not a GPU is present."""
    lib = _lib.lib
    c = config()
    a = np.zeros((33, 4), np.complex64)
    ptr = C.c_void_p(a.ctypes.data)
    assert lib.smx_phase_vocoder_c64(c._h, ptr, 1, 33, 4, 0.0, 0, ptr) == _lib.SMX_INVALID_ARGUMENT
    assert lib.smx_last_error().decode() == "phase_vocoder: cannot stretch by a rate of 0 (the rate must be finite and positive)"
    assert lib.smx_phase_vocoder_c128(c._h, ptr, 1, 32, 4, float("nan"), 1, ptr) == _lib.SMX_INVALID_ARGUMENT
    assert lib.smx_last_error().decode() == "phase_vocoder: cannot stretch by a rate of nan (the rate must be finite and positive)"
    assert lib.smx_phase_vocoder_c64_dev(c._h, ptr, 1, 32, 4, 1.5, 1, ptr, None) == _lib.SMX_INVALID_ARGUMENT
    assert lib.smx_last_error().decode() == ("phase_vocoder: cannot vocode 32 frequency bins of a 64-point transform (the bin axis "
                                             "must hold fft_size / 2 + 1 = 33 values)")
    assert lib.smx_time_stretch_f32(c._h, ptr, 1, 16, -2.0, 0, ptr) == _lib.SMX_INVALID_ARGUMENT
    assert lib.smx_last_error().decode() == "time_stretch: cannot stretch by a rate of -2 (the rate must be finite and positive)"
    assert lib.smx_time_stretch_f64(c._h, ptr, 1, 16, float("-inf"), 0, ptr) == _lib.SMX_INVALID_ARGUMENT
    assert lib.smx_last_error().decode() == "time_stretch: cannot stretch by a rate of -inf (the rate must be finite and positive)"
    gaps = Stft.Config.create(fft_size=64, hop=64)
    assert lib.smx_time_stretch_f32_dev(gaps._h, ptr, 1, 16, 1.5, 0, ptr, None) == _lib.SMX_INVALID_ARGUMENT
    assert lib.smx_last_error().decode().startswith("invert: cannot invert a 64-point window advanced by 64 samples")
    r = S.Resample.Config.create(3, 2)
    assert lib.smx_pitch_shift_f32(gaps._h, r._h, 0, ptr, 1, 16, ptr) == _lib.SMX_INVALID_ARGUMENT
    assert lib.smx_last_error().decode().startswith("invert: cannot invert a 64-point window advanced by 64 samples")
    count = C.c_int64()
    assert lib.smx_phase_vocoder_frames(9, 0.0, C.byref(count)) == _lib.SMX_INVALID_ARGUMENT
    assert lib.smx_time_stretch_length(9, float("inf"), C.byref(count)) == _lib.SMX_INVALID_ARGUMENT
    assert lib.smx_last_error().decode() == "time_stretch: cannot stretch by a rate of inf (the rate must be finite and positive)"


def test_zero_size_axes_touch_no_device():
    c = config()
    for shape in ((0, 33, 9), (33, 0), (2, 0, 33, 4)):
        for dtype in (np.complex64, np.complex128):
            for phase in ("independent", "locked"):
                out = Effects.phase_vocoder(c, np.zeros(shape, dtype), 1.37, phase=phase)
                assert out.dtype == dtype and out.shape == shape[:-1] + (R.out_frames(shape[-1], 1.37),)
    for shape, rate in (((0, 4000), 0.5), ((3, 0), 2.0), ((0,), 1.37), ((1,), 2.0), ((2, 1), 3.7)):
        for dtype in (np.float32, np.float64):
            y = Effects.time_stretch(c, np.zeros(shape, dtype), rate)
            assert y.dtype == dtype and y.shape == shape[:-1] + (R.stretch_length(shape[-1], rate),)
    for shape in ((0, 4000), (3, 0), (0,)):
        y = Effects.pitch_shift(c, np.zeros(shape, np.float32), (3, 2), phase="locked")
        assert y.dtype == np.float32 and y.shape == shape


def test_flat_reexports_and_defaults():
    import inspect
    for name in FACES:
        assert getattr(S, name) is getattr(Effects, name) and name in S.__all__
    assert "Effects" in S.__all__
    for name in ("phase_vocoder", "time_stretch", "pitch_shift"):
        assert inspect.signature(getattr(Effects, name)).parameters["phase"].default == "independent"
    assert inspect.signature(Effects.pitch_shift).parameters["quality"].default == "high"
    assert inspect.signature(Effects.semitones).parameters["bins_per_octave"].default == 12


def test_ctypes_signatures_agree_with_the_header():
    """Every Effects declaration: as many ctypes arguments as the header has parameters, int64 / double / int / pointer in the
    header's order."""
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "soundml_amd.h")).read(), flags=re.S)
    found = 0
    for m in re.finditer(r"\bint (smx_(?:phase_vocoder|time_stretch|pitch_shift|semitones)[a-z0-9_]*)\s*\(([^)]*)\)\s*;", header):
        name, params = m.group(1), [" ".join(p.split()) for p in m.group(2).split(",")]
        want = []
        for p in params:
            if p.startswith("int64_t *"):
                want.append(C.POINTER(C.c_int64))
            elif "*" in p:
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
        found += 1
    assert found == 13
