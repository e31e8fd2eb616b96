"""The host maps of ``Convert`` (convert.ml:104-115) and the argument checks of the decibel inverses (convert.ml:58-68): pinned values
(tests/golden/convert/pins.json), the laws of the grid maps, the reference's messages.  No GPU: the maps are host float64, and
the checks come before any device is looked for."""
import numpy as np
import pytest

import soundml_amd as S
from soundml_amd import Convert
from conftest import load_golden

PINS = load_golden("convert", "pins")


def test_midi_pins():
    p = PINS["hz_to_midi"]
    np.testing.assert_allclose(Convert.hz_to_midi(np.array(p["hz"])), p["midi"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(Convert.midi_to_hz(np.array(p["midi"])), p["hz"], rtol=1e-14, atol=0)


def test_time_to_frames_pin():
    p = PINS["time_to_frames"]
    got = Convert.time_to_frames(p["sample_rate"], p["hop"], np.array(p["times"]))
    assert got.dtype == np.float64
    assert got.tolist() == [float(v) for v in p["frames"]]


def test_frames_to_time_pin():
    p = PINS["frames_to_time"]
    got = Convert.frames_to_time(p["sample_rate"], p["hop"], np.array(p["frames"]))
    assert got.dtype == np.float64      # integer indices come back as float64 seconds
    np.testing.assert_allclose(got, p["times"], rtol=0, atol=1e-15)


def test_grid_round_trip_is_exact():
    """16384 / 512: a frame is 1 / 32 s, so every fourth frame index survives the trip through seconds exactly"""
    frames = 4.0 * np.arange(1024, dtype=np.float64)
    back = Convert.time_to_frames(16384, 512, Convert.frames_to_time(16384, 512, frames))
    assert np.array_equal(back, frames)


def test_midi_round_trip():
    hz = np.exp(np.linspace(np.log(20.0), np.log(20000.0), 64))
    np.testing.assert_allclose(Convert.midi_to_hz(Convert.hz_to_midi(hz)), hz, rtol=1e-12, atol=0)
    midi = Convert.hz_to_midi(hz)
    np.testing.assert_allclose(Convert.hz_to_midi(Convert.midi_to_hz(midi)), midi, rtol=1e-12, atol=0)


def test_shape_and_dtype_are_the_inputs():
    f = np.array([[110.0, 220.0, 440.0]], dtype=np.float32)
    for got in (Convert.hz_to_midi(f), Convert.midi_to_hz(f), Convert.frames_to_time(8000, 80, f), Convert.time_to_frames(8000, 80, f)):
        assert got.shape == f.shape and got.dtype == np.float32
    assert Convert.hz_to_midi(f).tolist() == [[45.0, 57.0, 69.0]]
    assert Convert.time_to_frames(8000, 80, np.array([0.0199, 0.02, -0.001])).tolist() == [1.0, 2.0, -1.0]     # the floor
    assert Convert.hz_to_midi(np.zeros((0, 3))).shape == (0, 3)


@pytest.mark.parametrize("fn", ["frames_to_time", "time_to_frames"])
def test_grid_messages(fn):
    v = np.arange(3.0)
    with pytest.raises(S.InvalidArgument) as e:
        getattr(Convert, fn)(0, 512, v)
    assert str(e.value) == "Soundml.Convert.%s: sample_rate must be positive" % fn
    with pytest.raises(S.InvalidArgument) as e:
        getattr(Convert, fn)(22050, 0, v)
    assert str(e.value) == "Soundml.Convert.%s: hop must be positive" % fn
    with pytest.raises(S.InvalidArgument) as e:     # the reference looks at the rate first
        getattr(Convert, fn)(-1, -1, v)
    assert str(e.value) == "Soundml.Convert.%s: sample_rate must be positive" % fn


@pytest.mark.parametrize("fn", ["db_to_power", "db_to_amplitude"])
@pytest.mark.parametrize("reference", [0.0, -1.0, float("inf"), float("nan")])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_reference_message(fn, reference, dtype):
    with pytest.raises(S.InvalidArgument) as e:
        getattr(Convert, fn)(np.zeros(4, dtype=dtype), reference=reference)
    assert str(e.value) == "Soundml.Convert.%s: reference must be finite and positive" % fn


def test_the_module_mirrors_all_of_convert():
    for name in ("power_to_db", "amplitude_to_db", "db_to_power", "db_to_amplitude", "hz_to_mel", "mel_to_hz", "hz_to_midi",
                 "midi_to_hz", "frames_to_time", "time_to_frames"):
        assert callable(getattr(Convert, name)), name
