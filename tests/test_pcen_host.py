"""What of Pcen runs without a device: the exports, every refusal word for word, the coefficient against the formula, the empty
results, the stream kernel's bookkeeping, and the header's naming rules for the smx_pcen entries."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import soundml_amd as S
from soundml_amd import Mel, Pcen, Stft, _lib

import pcen_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRAINED = "step: cannot feed a drained kernel (flush consumed the tail; reset before reusing)"
CARD = ["smx_pcen_apply_card_f32", "smx_pcen_kernel_step_card_f32", "smx_pcen_of_audio_card_f32", "smx_pcen_smooth_card_f32"]


def raises(message, fn, *args, **kw):
    with pytest.raises(S.InvalidArgument) as e:
        fn(*args, **kw)
    assert str(e.value) == message


def test_exports():
    assert S.Pcen is Pcen and S.pcen is Pcen.pcen
    for name in ("Pcen", "pcen"):
        assert name in S.__all__ and name in S.__doc__
    for name in ("Config", "apply", "smooth", "pcen", "Kernel", "TILE_MIN_FRAMES"):
        assert hasattr(Pcen, name), name
    assert Pcen.Kernel.latency == 0 and Pcen.TILE_MIN_FRAMES == 16


def test_create_refusals():
    create = Pcen.Config.create
    raises("create: cannot use a gain of -0.5 (gain must be at least 0)", create, gain=-0.5)
    raises("create: cannot use a bias of -1 (bias must be at least 0)", create, bias=-1.0)
    raises("create: cannot use a power of -2 (power must be at least 0)", create, power=-2.0)
    raises("create: cannot use an eps of 0 (eps must be positive)", create, eps=0.0)
    raises("create: cannot use an eps of -1e-06 (eps must be positive)", create, eps=-1e-6)
    raises("create: cannot use a time constant of 0 (time_constant must be positive)", create, time_constant=0.0)
    raises("create: cannot use a sample rate of 0 (sr must be at least 1)", create, sr=0)
    raises("create: cannot advance frames by -3 samples (hop must be at least 1)", create, hop=-3)
    raises("create: cannot smooth with the coefficient b = 1.5 (b must lie in [0, 1])", create, b=1.5)
    raises("create: cannot smooth with the coefficient b = -0.1 (b must lie in [0, 1])", create, b=-0.1)
    raises("create: cannot scale by 0 (scale must be positive)", create, scale=0.0)
    raises("create: cannot take the logarithm form without a bias (power == 0 needs bias > 0)", create, power=0.0, bias=0.0)
    for name in ("gain", "bias", "power", "time_constant", "eps", "b", "scale"):
        for bad, text in ((np.nan, "nan"), (np.inf, "inf")):
            raises("create: cannot use the parameter %s = %s (parameters must be finite)" % (name, text), create, **{name: bad})
    for b in (0.0, 1.0):
        assert create(b=b).coefficient == b


def test_coefficient_is_the_formula():
    for kw in (dict(), dict(sr=16000, hop=160), dict(time_constant=0.06), dict(sr=48000, hop=1024, time_constant=1.5), dict(b=0.025)):
        c = Pcen.Config.create(**kw)
        assert c.coefficient == R.coefficient(**R.params(**kw)), kw
    c = Pcen.Config.create(gain=0.8, scale=2.0 ** 31)
    assert (c.gain, c.scale, c.b, c.sr, c.hop) == (0.8, 2.0 ** 31, None, 22050, 512)


def test_rank_and_state_refusals():
    c = Pcen.Config.create()
    x = np.zeros((3, 4, 40), np.float32)
    for fn, op in ((Pcen.apply, "apply"), (Pcen.smooth, "smooth")):
        raises("%s: cannot normalise a tensor of rank 1 (the band and frame axes must exist: [...; bands; frames])" % op, fn, c, x[0, 0])
        raises("%s: cannot normalise a tensor of rank 0 (the band and frame axes must exist: [...; bands; frames])" % op, fn, c, np.asarray(1.0, np.float32))
        raises("%s: cannot start from a state of shape (3,) (zi must be one value per row, (3, 4))" % op, fn, c, x, np.zeros(3))
    raises("pcen: cannot analyse a rank-zero tensor (the time axis must exist)", Pcen.pcen, Stft.Config.create(fft_size=64),
           Mel.Config.create(n_mels=8, sample_rate=16000, fft_size=64), np.asarray(1.0, np.float32), c)


def test_device_float64_is_refused():
    """as energy.py words it; the check looks at the tensor alone, so a stand-in shows it without a device"""
    class Resident:
        device, bytes = True, 8
    from soundml_amd._tensor import refuse_device_float64
    assert Pcen.refuse_device_float64 is refuse_device_float64
    with pytest.raises(S.Failure) as e:
        Pcen.refuse_device_float64("apply", Resident(), "spectrograms are")
    assert str(e.value) == "apply: device-resident float64 spectrograms are not supported; pass a host array"


def test_empty_results_without_a_launch():
    c = Pcen.Config.create()
    for dtype in (np.float32, np.float64):
        out = Pcen.apply(c, np.ones((3, 4, 0), dtype))
        assert out.shape == (3, 4, 0) and out.dtype == dtype
        out, zf = Pcen.apply(c, np.ones((2, 0, 7), dtype), return_state=True)
        assert out.shape == (2, 0, 7) and zf.shape == (2, 0) and zf.dtype == np.float64
        z = np.arange(12.0).reshape(3, 4)
        out, zf = Pcen.apply(c, np.ones((3, 4, 0), dtype), zi=z, return_state=True)
        assert out.shape == (3, 4, 0) and np.array_equal(zf, z) and zf is not z
        assert Pcen.smooth(c, np.ones((0, 4, 9), dtype)).shape == (0, 4, 9)
    # the ABI's own empty spectrogram hands the state back too, before it asks for a device
    z = np.arange(5.0)
    zf = np.full(5, np.nan)
    assert _lib.lib.smx_pcen_apply_f32(c._h, None, 5, 0, C.c_void_p(z.ctypes.data), None, C.c_void_p(zf.ctypes.data)) == _lib.SMX_OK
    assert np.array_equal(zf, z)
    assert _lib.lib.smx_pcen_apply_f32(c._h, None, 5, 0, None, None, C.c_void_p(zf.ctypes.data)) == _lib.SMX_OK
    assert np.array_equal(zf, np.zeros(5))


def test_kernel_bookkeeping_on_shapes_alone():
    c = Pcen.Config.create()
    raises("prepare: cannot keep the state of 0 rows (rows must be at least 1)", Pcen.Kernel.prepare, c, 2, 0)
    raises("prepare: cannot keep the state of a stream without a band axis (lead_shape must end in the number of bands)", Pcen.Kernel.prepare, c)
    k = Pcen.Kernel.prepare(c, 2, 5)
    assert k.lead_shape == (2, 5) and Pcen.Kernel.prepare(c, (4,)).lead_shape == (4,)
    assert k.step(np.zeros((2, 5, 0), np.float32)) is None
    raises("step: cannot normalise a tensor of rank 1 (the band and frame axes must exist: [...; bands; frames])", k.step, np.zeros(4, np.float32))
    raises("step: cannot normalise a chunk of leading shape (3, 5) with a kernel prepared for (2, 5)", k.step, np.zeros((3, 5, 4), np.float32))
    assert k.flush() == [] and k.flush() == []
    raises(DRAINED, k.step, np.zeros((2, 5, 4), np.float32))
    raises(DRAINED, k.step, np.zeros((2, 5, 0), np.float32))
    k.reset()
    assert k.step(np.zeros((2, 5, 0), np.float32)) is None


def test_the_abi_checks_before_it_asks_for_a_device():
    lib = _lib.lib
    c = Pcen.Config.create()
    a = np.zeros(64, np.float32)
    ptr = C.c_void_p(a.ctypes.data)
    assert lib.smx_pcen_apply_card_f32(c._h, None, ptr, 1, 64, 32, None, ptr, None) == _lib.SMX_FAILURE
    assert lib.smx_last_error().decode() == "apply: x_stride is smaller than the number of frames"
    assert lib.smx_pcen_smooth_card_f32(c._h, None, ptr, 1, 64, 32, None, ptr) == _lib.SMX_FAILURE
    assert lib.smx_pcen_apply_f32(None, ptr, 1, 64, None, ptr, None) == _lib.SMX_FAILURE
    k = Pcen.Kernel.prepare(c, 1)
    assert lib.smx_pcen_kernel_step_card_f32(k._h, None, ptr, 64, 32, ptr) == _lib.SMX_FAILURE
    sc, mc = Stft.Config.create(fft_size=64), Mel.Config.create(n_mels=8, sample_rate=16000, fft_size=128)
    assert lib.smx_pcen_of_audio_card_f32(c._h, None, sc._h, mc._h, ptr, 1, 64, 64, ptr) == _lib.SMX_INVALID_ARGUMENT
    assert lib.smx_last_error().decode().startswith("mel_spectrogram: cannot project a 64-point STFT through a filterbank built for an FFT of size 128")
    handle = C.c_void_p()
    assert lib.smx_pcen_create(22050, 512, 0.98, 2.0, 0.5, 0.4, 0.0, 0, 0.0, 1.0, C.byref(handle)) == _lib.SMX_INVALID_ARGUMENT


def test_ctypes_signatures_agree_with_the_header():
    """every smx_pcen declaration: as many ctypes arguments as the header has parameters, of the header's kinds and in its order; the
    device-tensor entries end in _card_f32 and take the stream directly behind the first argument and a row pitch; no declaration
    matches a pattern by which an older suite collects entries"""
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "soundml_amd.h")).read(), flags=re.S)
    kinds = {"int64_t": C.c_int64, "double": C.c_double, "int": C.c_int}
    results = {"int": C.c_int, "int64_t": C.c_int64, "double": C.c_double, "void": None}
    found = {}
    for m in re.finditer(r"\b(int|int64_t|double|void) (smx_pcen[a-z0-9_]*)\s*\(([^)]*)\)\s*;", header):
        params = [" ".join(p.split()) for p in m.group(3).split(",")]
        found[m.group(2)] = params
        want = []
        for p in params:
            if p == "void":
                continue
            if p in ("smx_pcen **out", "smx_pcen_kernel **out"):
                want.append(C.POINTER(C.c_void_p))
            elif "*" in p:
                want.append(C.c_void_p)
            else:
                want.append(kinds[p.split(" ")[0]])
        res, args = _lib.SIGNATURES[m.group(2)]
        assert res is results[m.group(1)] and args == want, m.group(2)
    assert len(found) == 20 and set(found) == {n for n in _lib.SIGNATURES if n.startswith("smx_pcen")}
    taken = re.compile(r"_dev$|_dev_f(32|64)$|_device_f32$|_resident_f32$|_hbm_f32$|_accel_f32$|_gpu_f32$|_vram_f32$|^smx_iir_|^smx_loudness_")
    for name, params in found.items():
        assert not taken.search(name), name
        assert params[-1] != "void *stream", name
        if name.endswith("_card_f32"):
            assert params[1] == "void *stream" and "int64_t x_stride" in params, name
        else:
            assert not any("stream" in p for p in params), name
    assert sorted(n for n in found if n.endswith("_card_f32")) == CARD
    assert not re.findall(r"\b(smx_pcen\w+)\s*\([^;{}]*?void\s*\*\s*stream\s*\)\s*;", header)
