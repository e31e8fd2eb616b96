"""What of spectral contrast and onset strength runs without a device: the band plan (contrast.ml:60-142) against the
restatement over a grid, every Invalid_argument of contrast.ml and onset.ml word for word and in the reference's order, the
empty results, and the agreement of the ctypes signatures with the header."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import soundml_amd as S
from soundml_amd import Mel, Stft, _lib, contrast, onset

import contrast_onset_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")


def raises(message, fn, *args, **kw):
    with pytest.raises(S.InvalidArgument) as e:
        fn(*args, **kw)
    assert str(e.value) == message


# ---- the plan ---------------------------------------------------------------------------------------------------------------

def test_the_two_default_plans():
    assert contrast.plan(6, 200.0, 0.02, 22050, 2048) == [(0, 18, 1), (18, 19, 1), (37, 37, 1), (74, 74, 2), (148, 149, 3),
                                                          (297, 297, 6), (594, 431, 9)]
    assert contrast.plan(6, 200.0, 0.02, 48000, 2048)[-1] == (273, 752, 15)
    assert [contrast.plan(6, 200.0, q, 22050, 2048)[-1][2] for q in (0.0375, 0.04, 0.5)] == [16, 17, 216]


@pytest.mark.parametrize("sample_rate", [8000, 16000, 22050, 48000])
def test_plan_grid(sample_rate):
    """the library's plan is the restatement's, and refuses what the restatement refuses in the same words"""
    kept = 0
    for fft_size in (128, 400, 512, 2048, 4096):
        for n_bands in range(1, 8):
            for quantile in (0.02, 0.0375, 0.04, 0.31, 0.5, 0.97):
                try:
                    want = R.plan(n_bands, 200.0, quantile, sample_rate, fft_size)
                except R.Rejected as e:
                    raises("spectral_contrast: %s" % e, contrast.plan, n_bands, 200.0, quantile, sample_rate, fft_size)
                    continue
                assert contrast.plan(n_bands, 200.0, quantile, sample_rate, fft_size) == want, (fft_size, n_bands, quantile)
                assert all(1 <= take <= sub_len for _, sub_len, take in want)
                kept += 1
    assert kept >= 100


def test_rint_rounds_half_to_even():
    """quantile * count on a tie goes to the even neighbour (contrast.ml:52-58), not away from zero"""
    for n_bands, quantile in ((1, 0.25), (2, 0.25), (3, 0.5)):
        assert contrast.plan(n_bands, 200.0, quantile, 8000, 128) == R.plan(n_bands, 200.0, quantile, 8000, 128)
    assert R.rint(6.5) == 6.0 and R.rint(7.5) == 8.0 and R.rint(0.5) == 0.0


# ---- messages ---------------------------------------------------------------------------------------------------------------

PLAN_CASES = [
    (dict(n_bands=0, f_min=-1.0, quantile=2.0, sample_rate=0), "cannot divide the spectrum into 0 octave bands (n_bands must be at least 1)"),
    (dict(n_bands=-3), "cannot divide the spectrum into -3 octave bands (n_bands must be at least 1)"),
    (dict(f_min=-1.0, quantile=2.0, sample_rate=0), "cannot start the first octave band at -1 Hz (f_min must be finite and positive)"),
    (dict(f_min=0.0), "cannot start the first octave band at 0 Hz (f_min must be finite and positive)"),
    (dict(f_min=NAN), "cannot start the first octave band at nan Hz (f_min must be finite and positive)"),
    (dict(f_min=float("inf")), "cannot start the first octave band at inf Hz (f_min must be finite and positive)"),
    (dict(quantile=1.0, sample_rate=0), "cannot average the 1 quantile of each band (quantile must lie strictly between 0 and 1)"),
    (dict(quantile=0.0), "cannot average the 0 quantile of each band (quantile must lie strictly between 0 and 1)"),
    (dict(quantile=NAN), "cannot average the nan quantile of each band (quantile must lie strictly between 0 and 1)"),
    (dict(sample_rate=0, n_bands=40), "cannot use a sample rate of 0 Hz (sample_rate must be at least 1)"),
    (dict(n_bands=7), "cannot start the top octave band at 12800 Hz at a sample rate of 22050 Hz (every band must start below the Nyquist "
                      "frequency 11025; lower f_min or n_bands)"),
    (dict(f_min=20.0), "cannot resolve the octave band [0, 20] Hz with an FFT of size 512 at a sample rate of 22050 Hz (the band spans no FFT "
                       "bin below its top edge; raise fft_size or lower n_bands)"),
]


def contrast_call(fn, kw, bad_rank=False, bins=257):
    kw = dict(dict(sample_rate=22050), **kw)
    c = Stft.Config.create(fft_size=512, hop=128)
    if fn == "spectral_contrast":
        return S.spectral_contrast(c, np.asarray(1.0, np.float32) if bad_rank else np.zeros(2000, np.float32), **kw)
    if fn == "spectral_contrast_of_spectrogram":
        return S.spectral_contrast_of_spectrogram(np.ones(5 if bad_rank else (bins, 4), np.float32), **kw)
    stage = S.spectral_contrast_stage(c, **kw)
    return stage.step(np.ones(5 if bad_rank else (bins, 4), np.float32))


@pytest.mark.parametrize("fn", ["spectral_contrast", "spectral_contrast_of_spectrogram", "spectral_contrast_stage"])
def test_contrast_messages_in_the_reference_order(fn):
    flat = fn == "spectral_contrast_of_spectrogram"
    for kw, message in PLAN_CASES:
        raises("%s: %s" % (fn, message), contrast_call, fn, kw)
        if not flat:         # the plan is built before the tensor is looked at (contrast.ml:211-217, 257-261)
            raises("%s: %s" % (fn, message), contrast_call, fn, kw, bad_rank=True)
    if fn == "spectral_contrast":
        raises("spectral_contrast: cannot analyse a rank-zero tensor (the time axis must exist)", contrast_call, fn, {}, bad_rank=True)
        return
    # contrast.ml:226-232 / 157-162: the rank comes first in the spectrogram-input mode, before every parameter
    rank = "%s: cannot analyse a rank-1 tensor (spectral contrast needs [...; bins; frames])" % fn
    raises(rank, contrast_call, fn, {}, bad_rank=True)
    if flat:
        raises(rank, contrast_call, fn, dict(n_bands=0), bad_rank=True)
        few = ("%s: cannot derive bin frequencies for a %d-bin spectrogram (the implied FFT size is %d; a magnitude spectrogram holds "
               "fft_size / 2 + 1 bins)")
        raises(few % (fn, 1, 0), contrast_call, fn, dict(n_bands=0), bins=1)
        raises(few % (fn, 0, -2), contrast_call, fn, {}, bins=0)
    else:
        raises("%s: cannot band 100 frequency bins with a plan built for an FFT of size 512 (257 bins)" % fn, contrast_call, fn, {}, bins=100)


def test_onset_messages_in_the_reference_order():
    c = Stft.Config.create(fft_size=512, hop=128)
    mc, other = Mel.Config.create(n_mels=40, sample_rate=22050, fft_size=512), Mel.Config.create(n_mels=40, sample_rate=22050, fft_size=256)
    x, scalar = np.zeros(2000, np.float32), np.asarray(1.0, np.float32)
    lag = "%s: cannot difference frames at a lag of %d (lag must be at least 1)"
    raises(lag % ("onset_strength", 0), S.onset_strength, c, other, scalar, lag=0)
    raises(lag % ("onset_strength", -2), S.onset_strength, c, mc, x, lag=-2)
    raises("onset_strength: cannot project a 512-point STFT through a filterbank built for an FFT of size 256 (the two configurations "
           "must agree on fft_size)", S.onset_strength, c, other, scalar)
    raises("onset_strength: cannot analyse a rank-zero tensor (the time axis must exist)", S.onset_strength, c, mc, scalar)
    raises(lag % ("onset_strength_stage", 0), S.onset_strength_stage, 0)
    stage = S.onset_strength_stage(lag=2)
    raises("onset_strength_stage: cannot aggregate a rank-1 tensor (the onset flux needs [...; bins; frames])", stage.step, np.zeros(5, np.float32))
    zero = "onset_strength_stage: cannot aggregate a chunk with a zero-size axis (bins and channels must be at least 1)"
    raises(zero, stage.step, np.zeros((0, 9), np.float32))
    raises(zero, stage.step, np.zeros((0, 4, 9), np.float64))
    raises(zero, stage.step, np.zeros((2, 0, 0), np.float32))


def test_the_abi_checks_before_it_asks_for_a_device():
    """The C entry points word the same errors themselves, before require_device: SMX_INVALID_ARGUMENT, not the missing-device
    Failure, whether or not a GPU is present."""
    lib = _lib.lib
    a = np.zeros((257, 4), np.float32)
    ptr = C.c_void_p(a.ctypes.data)
    c = Stft.Config.create(fft_size=512, hop=128)
    mc = Mel.Config.create(n_mels=40, sample_rate=22050, fft_size=256)
    assert lib.smx_spectral_contrast_f32(c._h, ptr, 1, 1000, 6, 200.0, 0.02, 0, 0, ptr) == _lib.SMX_INVALID_ARGUMENT
    assert lib.smx_last_error().decode() == "spectral_contrast: cannot use a sample rate of 0 Hz (sample_rate must be at least 1)"
    assert lib.smx_spectral_contrast_of_spectrogram_f64(ptr, 1, 1, 4, 0, 6, 200.0, 0.02, 0, 22050, 1, ptr) == _lib.SMX_INVALID_ARGUMENT
    assert lib.smx_last_error().decode().startswith("spectral_contrast_of_spectrogram: cannot derive bin frequencies for a 1-bin spectrogram")
    assert lib.smx_spectral_contrast_of_spectrogram_f32(ptr, 1, 100, 4, 512, 6, 200.0, 0.02, 0, 22050, 0, ptr) == _lib.SMX_INVALID_ARGUMENT
    assert lib.smx_last_error().decode() == "spectral_contrast_stage: cannot band 100 frequency bins with a plan built for an FFT of size 512 (257 bins)"
    assert lib.smx_onset_strength_f32(c._h, mc._h, ptr, 1, 1000, 1, ptr) == _lib.SMX_INVALID_ARGUMENT
    assert lib.smx_last_error().decode().startswith("onset_strength: cannot project a 512-point STFT through a filterbank built for an FFT of size 256")
    assert lib.smx_onset_flux_f64(ptr, 1, 4, 4, 0, ptr) == _lib.SMX_INVALID_ARGUMENT
    assert lib.smx_last_error().decode() == "onset_strength_stage: cannot difference frames at a lag of 0 (lag must be at least 1)"
    assert lib.smx_onset_flux_f32(ptr, 1, 0, 4, 1, ptr) == _lib.SMX_INVALID_ARGUMENT


# ---- empty shapes -----------------------------------------------------------------------------------------------------------

def test_zero_size_axes_touch_no_device():
    c = Stft.Config.create(fft_size=512, hop=128)
    left = Stft.Config.create(fft_size=512, hop=128, alignment="left")
    mc = Mel.Config.create(n_mels=40, sample_rate=22050, fft_size=512)
    assert Stft.frames(left, 100) == 0
    for dtype in (np.float32, np.float64):
        for shape in ((0, 257, 9), (2, 257, 0), (0, 3, 257, 0)):
            out = S.spectral_contrast_of_spectrogram(np.zeros(shape, dtype), sample_rate=22050)
            assert out.shape == shape[:-2] + (7, shape[-1]) and out.dtype == dtype
            out = S.spectral_contrast_stage(c, sample_rate=22050, n_bands=4).step(np.zeros(shape, dtype))
            assert out.shape == shape[:-2] + (5, shape[-1]) and out.dtype == dtype
        out = S.spectral_contrast(c, np.zeros((0, 4000), dtype), sample_rate=22050)
        assert out.shape == (0, 7, Stft.frames(c, 4000)) and out.dtype == dtype
        out = S.spectral_contrast(left, np.zeros((3, 100), dtype), sample_rate=22050, n_bands=3)
        assert out.shape == (3, 4, 0) and out.dtype == dtype
        out = S.onset_strength(c, mc, np.zeros((0, 4000), dtype))
        assert out.shape == (0, Stft.frames(c, 4000)) and out.dtype == dtype
        out = S.onset_strength(left, mc, np.zeros((2, 3, 100), dtype), lag=4)
        assert out.shape == (2, 3, 0) and out.dtype == dtype
        stage = S.onset_strength_stage(lag=2)
        out = stage.step(np.zeros((2, 40, 0), dtype))
        assert out.shape == (2, 0) and out.dtype == dtype and stage.flush() == [] and stage.latency == 0


def test_flat_reexports_and_defaults():
    import inspect
    for name, module in (("spectral_contrast", contrast), ("spectral_contrast_of_spectrogram", contrast), ("spectral_contrast_stage", contrast),
                         ("onset_strength", onset), ("onset_strength_stage", onset)):
        assert getattr(S, name) is getattr(module, name) and name in S.__all__
        sig = inspect.signature(getattr(module, name))
        if "contrast" in name:
            assert [sig.parameters[k].default for k in ("n_bands", "f_min", "quantile", "linear")] == [6, 200.0, 0.02, False]
        else:
            assert sig.parameters["lag"].default == 1


# ---- signatures -------------------------------------------------------------------------------------------------------------

def test_ctypes_signatures_agree_with_the_header():
    """Every smx_spectral_contrast* / smx_onset_* declaration: as many ctypes arguments as the header has parameters, int64 /
    double / int / pointer in the header's order; the device forms carry the dtype last and take a stream."""
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "soundml_amd.h")).read(), flags=re.S)
    found = []
    for m in re.finditer(r"\bint (smx_(?:spectral_contrast|onset)_?[a-z0-9_]*)\s*\(([^)]*)\)\s*;", header):
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
        if "_dev" in name:
            assert name.endswith("_dev_f32") and params[-1] == "void *stream", name
        found.append(name)
    assert len(found) == 13 and len([n for n in found if n.endswith("_dev_f32")]) == 4, found
