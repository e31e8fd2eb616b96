"""What of Loudness runs without a device: the exports, the shapes of the results that need no launch (zero-size leading axes,
n = 0, fewer samples than one gating block), every refusal word for word, the meter's bookkeeping on shapes alone, and the
header's naming rules for the smx_loudness_ entries."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import soundml_amd as S
from soundml_amd import Loudness, _lib

import loudness_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATE = 48000
BLOCK = 4 * R.step(RATE)


def raises(message, fn, *args, **kw):
    with pytest.raises(S.InvalidArgument) as e:
        fn(*args, **kw)
    assert str(e.value) == message


def test_exports():
    assert S.Loudness is Loudness and S.loudness is Loudness.integrated and S.true_peak is Loudness.true_peak
    for name in ("Loudness", "loudness", "true_peak"):
        assert name in S.__all__ and name in S.__doc__, name
    for name in ("k_weighting", "true_peak_taps", "block_energy", "momentary", "short_term", "integrated", "true_peak", "normalize", "Meter",
                 "gate_mask", "SURROUND_5_0", "ABSOLUTE_GATE", "MIN_RATE", "MAX_CHANNELS"):
        assert hasattr(Loudness, name), name
    assert (Loudness.MIN_RATE, Loudness.MAX_CHANNELS) == (8000, 32)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_shapes_that_need_no_launch(dtype):
    for lead in ((), (3,), (0,), (2, 0)):
        for n in (0, BLOCK - 1):
            x = np.ones(lead + (2, n), dtype)
            z = Loudness.block_energy(x, RATE)
            assert z.shape == lead + (2, 0) and z.dtype == np.float64
            m = Loudness.momentary(x, RATE)
            assert m.shape == lead + (0,) and m.dtype == dtype
            assert Loudness.short_term(x, RATE).shape == lead + (0,)
            i = Loudness.integrated(x, RATE)
            assert i.shape == lead and i.dtype == dtype and np.all(np.isneginf(i))
            assert Loudness.gate_mask(x, RATE).shape == lead + (0,)
        for n in (BLOCK, BLOCK + 1, BLOCK + R.step(RATE), 30 * R.step(RATE)):
            nb = Loudness.blocks(RATE, n)
            assert nb == (1, 1, 2, 27)[(BLOCK, BLOCK + 1, BLOCK + R.step(RATE), 30 * R.step(RATE)).index(n)]
            if 0 in lead:
                x = np.ones(lead + (2, n), dtype)
                assert Loudness.block_energy(x, RATE).shape == lead + (2, nb)
                assert Loudness.momentary(x, RATE).shape == lead + (nb,)
                assert Loudness.short_term(x, RATE).shape == lead + (max(0, nb - 26),)
                assert Loudness.integrated(x, RATE).shape == lead
                assert Loudness.normalize(x, RATE).shape == x.shape
                assert Loudness.true_peak(x).shape == lead + (2,)
        x = np.ones(lead + (2, 0), dtype)
        p = Loudness.true_peak(x)
        assert p.shape == lead + (2,) and p.dtype == dtype and np.all(p == 0)
        assert Loudness.normalize(x, RATE).shape == x.shape


def test_refusals():
    x = np.zeros((2, 100), np.float32)
    for fn, op in ((Loudness.block_energy, "block_energy"), (Loudness.momentary, "momentary"), (Loudness.short_term, "short_term"),
                   (Loudness.integrated, "integrated"), (Loudness.normalize, "normalize")):
        raises("%s: cannot meter audio at 7999 Hz (rate must be at least 8000)" % op, fn, x, 7999)
        raises("%s: cannot meter a tensor of shape (100,) (audio is [...; channels; n]: the channel axis must exist, [1; n] for mono)" % op,
               fn, x[0], RATE)
        raises("%s: cannot analyse a rank-zero tensor (the time axis must exist)" % op, fn, np.asarray(1.0, np.float32), RATE)
        raises("%s: cannot meter 33 channels (channels must lie in [1, 32])" % op, fn, np.zeros((33, 10), np.float32), RATE)
        raises("%s: cannot meter 0 channels (channels must lie in [1, 32])" % op, fn, np.zeros((0, 10), np.float32), RATE)
    raises("k_weighting: cannot weight audio at 7999 Hz (rate must be at least 8000)", Loudness.k_weighting, 7999)
    raises("true_peak: cannot meter a tensor of shape (100,) (audio is [...; channels; n]: the channel axis must exist, [1; n] for mono)",
           Loudness.true_peak, x[0])
    for fn, op in ((Loudness.momentary, "momentary"), (Loudness.short_term, "short_term"), (Loudness.integrated, "integrated"),
                   (Loudness.normalize, "normalize")):
        raises("%s: cannot weight 2 channels with 5 weights (weights must have one entry per channel)" % op, fn, x, RATE,
               weights=Loudness.SURROUND_5_0)
    raises("normalize: cannot hold peaks under 0 (peak_ceiling is a linear amplitude: positive and finite)", Loudness.normalize, x, RATE, peak_ceiling=0.0)
    raises("prepare: cannot meter audio at 4000 Hz (rate must be at least 8000)", Loudness.Meter.prepare, 4000, 2)
    raises("prepare: cannot weight 2 channels with 1 weights (weights must have one entry per channel)", Loudness.Meter.prepare, RATE, 2, weights=[1.0])
    raises("prepare: cannot keep the state of 0 clips (the leading axes must not be empty)", Loudness.Meter.prepare, RATE, 0, 2)


def test_the_abi_words_its_own_refusals_before_it_asks_for_a_device():
    lib = _lib.lib
    a = np.zeros(64, np.float32)
    ptr = C.c_void_p(a.ctypes.data)
    assert lib.smx_loudness_integrated_card_f32(ptr, None, 1, 2, 32, 32, 4000, None, ptr, None) == _lib.SMX_INVALID_ARGUMENT
    assert lib.smx_last_error().decode() == "integrated: cannot meter audio at 4000 Hz (rate must be at least 8000)"
    assert lib.smx_loudness_momentary_f32(ptr, 1, 40, 1, RATE, None, 0, ptr) == _lib.SMX_INVALID_ARGUMENT
    assert lib.smx_last_error().decode() == "momentary: cannot meter 40 channels (channels must lie in [1, 32])"
    w = np.array([1.0, -1.0])
    assert lib.smx_loudness_integrated_f32(ptr, 1, 2, 32, RATE, C.c_void_p(w.ctypes.data), ptr, None) == _lib.SMX_INVALID_ARGUMENT
    assert lib.smx_last_error().decode() == "integrated: cannot weight channel 1 by -1 (weights must be finite and not negative)"
    assert lib.smx_loudness_true_peak_card_f32(ptr, None, 1, 64, 32, ptr) == _lib.SMX_FAILURE
    assert lib.smx_loudness_block_energy_card_f32(ptr, None, 1, 2, 32, 16, RATE, ptr) == _lib.SMX_FAILURE


def test_device_float64_is_refused():
    """as iir.py words it; the check looks at the tensor alone, so a stand-in shows it without a device"""
    class Resident:
        device, bytes = True, 8
    for op in ("block_energy", "momentary", "integrated", "true_peak", "normalize", "step"):
        with pytest.raises(S.Failure) as e:
            Loudness._refuse_device_float64(op, Resident())
        assert str(e.value) == "%s: device-resident float64 audio is not supported; pass a host array" % op


def test_meter_bookkeeping_on_shapes_alone():
    k = Loudness.Meter.prepare(RATE, 3, 2)
    assert k.lead_shape == (3,) and k.channels == 2 and k.position == 0 and k.blocks == 0
    assert Loudness.Meter.prepare(RATE, (2,)).lead_shape == ()
    assert k.step(np.zeros((3, 2, 0), np.float32)) is None and k.position == 0
    raises("step: cannot meter a chunk of leading shape (2, 2) with a meter prepared for (3, 2)", k.step, np.zeros((2, 2, 4), np.float32))
    raises("step: cannot meter a tensor of shape (4,) (chunks are [...; channels; m])", k.step, np.zeros(4, np.float32))
    i = k.integrated()
    assert i.shape == (3,) and np.all(np.isneginf(i))          # nothing fed: nothing through the gates... and no launch
    assert k.short_term().shape == (3, 0)
    assert k.flush() == [] and k.flush() == []
    drained = "step: cannot feed a drained meter (flush closed the stream; reset before reusing)"
    raises(drained, k.step, np.zeros((3, 2, 4), np.float32))
    raises(drained, k.step, np.zeros((3, 2, 0), np.float32))
    k.reset()
    assert k.step(np.zeros((3, 2, 0), np.float32)) is None


def test_header_naming_rules():
    """the device-tensor entries end in _card_f32 and take the stream directly behind the first argument; no smx_loudness_ declaration
    matches a pattern by which an older suite collects entries, and every declaration has its ctypes row with as many arguments"""
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "soundml_amd.h")).read(), flags=re.S)
    found = {}
    for m in re.finditer(r"\b(?:int|int64_t|void|double) (smx_loudness_[a-z0-9_]*)\s*\(([^)]*)\)\s*;", header):
        found[m.group(1)] = [p.strip() for p in m.group(2).split(",")]
    assert len(found) == 33 and set(found) == {n for n in _lib.SIGNATURES if n.startswith("smx_loudness_")}
    taken = re.compile(r"_dev$|_dev_f(32|64)$|_device_f32$|_resident_f32$|_hbm_f32$|_accel_f32$|_gpu_f32$|_vram_f32$")
    for name, params in found.items():
        assert not taken.search(name), name
        assert params[-1] != "void *stream", name
        assert len(_lib.SIGNATURES[name][1]) == (0 if params == ["void"] else len(params)), name
        if name.endswith("_card_f32"):
            assert params[1] == "void *stream", name
        else:
            assert not any("stream" in p for p in params), name
    assert sorted(n for n in found if n.endswith("_card_f32")) == [
        "smx_loudness_block_energy_card_f32", "smx_loudness_integrated_card_f32", "smx_loudness_meter_read_card_f32", "smx_loudness_meter_step_card_f32",
        "smx_loudness_momentary_card_f32", "smx_loudness_normalize_card_f32", "smx_loudness_true_peak_card_f32"]
