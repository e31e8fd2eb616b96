"""What of Hpss runs without a device: the argument checks (hpss.ml:351-403, 477-486: kernel, power, margin, rank, dtype, in
that order, before any device work), the empty results, and the agreement of the ctypes signatures with the header."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import soundml_amd as S
from soundml_amd import Hpss, Stft, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")

FACES = ["hpss_masks", "hpss_of_spectrogram", "hpss_of_stft", "hpss", "harmonic", "percussive"]


def call(fn, bad_rank=False, dtype=np.float32, **kw):
    if fn in ("hpss", "harmonic", "percussive"):
        c = Stft.Config.create(fft_size=512, hop=128)
        x = np.asarray(1.0, dtype) if bad_rank else np.zeros(2000, dtype)
        return getattr(Hpss, fn)(c, x, **kw)
    s = np.ones(5 if bad_rank else (4, 4), np.complex64 if fn == "hpss_of_stft" else dtype)
    return getattr(Hpss, fn)(s, **kw)


@pytest.mark.parametrize("fn", FACES)
def test_messages_in_the_reference_order(fn):
    cases = [
        (dict(kernel_size=(0, 31), power=-1.0, margin=(0.0, 0.0), bad_rank=True),
         "cannot median-filter with a kernel of (0, 31) (both kernel sizes must be at least 1)"),
        (dict(kernel_size=(31, -4)), "cannot median-filter with a kernel of (31, -4) (both kernel sizes must be at least 1)"),
        (dict(power=0.0, margin=(0.5, 1.0), bad_rank=True),
         "cannot raise the mask to the power 0 (power must be strictly positive, or infinite for a hard mask)"),
        (dict(power=-2.5), "cannot raise the mask to the power -2.5 (power must be strictly positive, or infinite for a hard mask)"),
        (dict(power=float("nan")), "cannot raise the mask to the power nan (power must be strictly positive, or infinite for a hard mask)"),
        (dict(margin=(1.0, 0.5), bad_rank=True), "cannot bias the decision by a margin of (1, 0.5) (both margins must be finite and at least 1)"),
        (dict(margin=(INF, 2.0)), "cannot bias the decision by a margin of (inf, 2) (both margins must be finite and at least 1)"),
        (dict(margin=(float("nan"), 1.0)), "cannot bias the decision by a margin of (nan, 1) (both margins must be finite and at least 1)"),
    ]
    for kw, message in cases:
        with pytest.raises(S.InvalidArgument) as e:
            call(fn, **kw)
        assert str(e.value) == "%s: %s" % (fn, message)
    with pytest.raises(S.InvalidArgument) as e:
        call(fn, bad_rank=True)
    if fn in ("hpss", "harmonic", "percussive"):
        assert str(e.value) == "%s: cannot separate a rank-zero tensor (the time axis must exist)" % fn
    else:
        assert str(e.value) == "%s: cannot separate a rank-1 tensor (a spectrogram carries a bin axis and a frame axis)" % fn
    if fn != "hpss_of_stft":
        with pytest.raises(S.InvalidArgument) as e:
            call(fn, dtype=np.float16)
        assert str(e.value) == "%s: cannot separate float16 spectra (the median kernel carries float32 and float64)" % fn


def test_the_abi_checks_before_it_asks_for_a_device():
    """The C entry points word the same errors themselves, before require_device: SMX_INVALID_ARGUMENT, not the
    missing-device Failure, whether or not a GPU is present."""
    lib = _lib.lib
    a = np.zeros((4, 4), np.float32)
    ptr = C.c_void_p(a.ctypes.data)
    assert lib.smx_hpss_masks_f32(ptr, 1, 4, 4, 31, 0, 2.0, 1.0, 1.0, ptr, ptr) == _lib.SMX_INVALID_ARGUMENT
    assert lib.smx_last_error().decode() == "hpss_masks: cannot median-filter with a kernel of (31, 0) (both kernel sizes must be at least 1)"
    assert lib.smx_hpss_of_spectrogram_f64(ptr, 1, 4, 4, 31, 31, float("nan"), 1.0, 1.0, ptr, ptr) == _lib.SMX_INVALID_ARGUMENT
    assert lib.smx_last_error().decode() == ("hpss_of_spectrogram: cannot raise the mask to the power nan (power must be strictly "
                                             "positive, or infinite for a hard mask)")
    assert lib.smx_hpss_of_stft_c64(ptr, 1, 4, 2, 31, 31, INF, 1.0, 0.0, ptr, ptr) == _lib.SMX_INVALID_ARGUMENT
    assert lib.smx_last_error().decode() == ("hpss_of_stft: cannot bias the decision by a margin of (1, 0) (both margins must be "
                                             "finite and at least 1)")
    c = Stft.Config.create(fft_size=512, hop=128)
    assert lib.smx_hpss_f32(c._h, ptr, 1, 16, 0, 0, 2.0, 1.0, 1.0, None, ptr) == _lib.SMX_INVALID_ARGUMENT
    assert lib.smx_last_error().decode() == "percussive: cannot median-filter with a kernel of (0, 0) (both kernel sizes must be at least 1)"
    # Stft.invert's own preconditions come with the signal face: a rectangular 16-point window advanced by 32 leaves gaps
    gaps = Stft.Config.create(fft_size=32, win_length=16, hop=32, window="rectangular")
    assert lib.smx_hpss_f32(gaps._h, ptr, 1, 16, 31, 31, 2.0, 1.0, 1.0, ptr, ptr) == _lib.SMX_INVALID_ARGUMENT
    assert lib.smx_last_error().decode().startswith("invert: cannot invert a 16-point window advanced by 32 samples")


def test_zero_size_axes_touch_no_device():
    for shape in ((0, 9, 9), (2, 0, 9), (2, 9, 0), (0, 7)):
        for dtype in (np.float32, np.float64):
            for face in (Hpss.hpss_masks, Hpss.hpss_of_spectrogram):
                a, b = face(np.zeros(shape, dtype))
                assert a.shape == shape and b.shape == shape and a.dtype == dtype
        z_h, z_p = Hpss.hpss_of_stft(np.zeros(shape, np.complex128))
        assert z_h.shape == shape and z_p.dtype == np.complex128
    c = Stft.Config.create(fft_size=512, hop=128)
    for shape in ((0, 4000), (3, 0)):
        y_h, y_p = Hpss.hpss(c, np.zeros(shape, np.float32))
        assert y_h.shape == shape and y_p.shape == shape
        assert Hpss.harmonic(c, np.zeros(shape, np.float64)).dtype == np.float64


def test_flat_reexports_and_defaults():
    import inspect
    for name in FACES:
        assert getattr(S, name) is getattr(Hpss, name) and name in S.__all__
        sig = inspect.signature(getattr(Hpss, name))
        assert sig.parameters["kernel_size"].default == (31, 31)
        assert sig.parameters["power"].default == 2.0 and sig.parameters["margin"].default == (1.0, 1.0)
    assert "Hpss" in S.__all__


def test_ctypes_signatures_agree_with_the_header():
    """Every smx_hpss_* declaration: as many ctypes arguments as the header has parameters, int64 / double / pointer in the
    header's order."""
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "soundml_amd.h")).read(), flags=re.S)
    found = 0
    for m in re.finditer(r"\bint (smx_hpss_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", header):
        name, params = m.group(1), [p.strip() for p in m.group(2).split(",")]
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
        found += 1
    assert found == 12
