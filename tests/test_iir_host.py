"""What of Iir runs without a device: the exports and constants, every refusal word for word, the host-built tables against the
restatement bit for bit, the empty results, and the header's naming rules for the smx_iir_ entries."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import soundml_amd as S
from soundml_amd import Iir, _lib

import iir_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRAINED = "step: cannot feed a drained kernel (flush consumed the tail; reset before reusing)"


def raises(message, fn, *args, **kw):
    with pytest.raises(S.InvalidArgument) as e:
        fn(*args, **kw)
    assert str(e.value) == message


def test_exports_and_constants():
    assert S.Iir is Iir and "Iir" in S.__all__ and "Iir" in S.__doc__
    for name in ("Config", "apply", "filtfilt", "zi", "Kernel", "BLOCK", "SPAN_BLOCKS", "MAX_SECTIONS"):
        assert hasattr(Iir, name), name
    assert (Iir.BLOCK, Iir.SPAN_BLOCKS, Iir.MAX_SECTIONS) == (R.BLOCK, R.SPAN_BLOCKS, R.MAX_SECTIONS) == (256, 64, 8)
    assert Iir.BLOCK % 2 == 0 and Iir.BLOCK & (Iir.BLOCK - 1) == 0
    assert Iir.Kernel.latency == 0


def test_create_refusals():
    ok = R.cascade(2)
    raises("create: cannot run a cascade of 0 sections (sections must lie in [1, 8])", Iir.Config.create, np.zeros((0, 6)))
    raises("create: cannot run a cascade of 9 sections (sections must lie in [1, 8])", Iir.Config.create, R.cascade(9))
    raises("create: cannot read an array of shape (6,) as second-order sections (sos must be [sections; 6])", Iir.Config.create, ok[0])
    raises("create: cannot read an array of shape (2, 5) as second-order sections (sos must be [sections; 6])", Iir.Config.create, ok[:, :5])
    bad = ok.copy()
    bad[1, 3] = 2.0
    raises("create: cannot run section 1 with a0 = 2 (sections must be normalised: a0 must be exactly 1)", Iir.Config.create, bad)
    bad[1, 3] = np.nextafter(1.0, 2.0)
    raises("create: cannot run section 1 with a0 = 1 (sections must be normalised: a0 must be exactly 1)", Iir.Config.create, bad)
    bad = ok.copy()
    bad[0, 1] = np.nan
    raises("create: cannot use the coefficient nan of section 0 (coefficients must be finite)", Iir.Config.create, bad)


def test_tables_are_the_restatement_bit_for_bit():
    for s in (1, 2, 3, 4, 8):
        sos = R.cascade(s)
        c = Iir.Config.create(sos)
        assert c.sections == s and c.padlen == R.padlen(sos)
        assert np.array_equal(c.matrix, R.matrix(sos))
        assert np.array_equal(Iir.zi(c), R.zi(sos)) and Iir.zi(c).shape == (s, 2)
    # padlen counts the sections of first order: scipy's ntaps
    first_order = np.array([[1.0, -1.0, 0.0, 1.0, -0.995, 0.0], [0.2, 0.2, 0.0, 1.0, -0.6, 0.0], [1.0, 0.5, 0.25, 1.0, -0.5, 0.1]])
    assert Iir.Config.create(first_order).padlen == 3 * (2 * 3 + 1 - 2) == R.padlen(first_order)


def test_zi_refuses_a_pole_at_one():
    integrator = np.array([[1.0, 0.0, 0.0, 1.0, -0.5, 0.0], [1.0, 0.0, 0.0, 1.0, -1.0, 0.0]])
    c = Iir.Config.create(integrator)
    message = "zi: cannot settle section 1 on a unit step (1 + a1 + a2 is zero: a pole at z = 1)"
    raises(message, Iir.zi, c)
    raises(message, Iir.filtfilt, c, np.zeros(100, np.float32))


def test_apply_and_filtfilt_refusals():
    c = Iir.Config.create(R.cascade(2))
    x = np.zeros((3, 40), np.float32)
    raises("apply: cannot analyse a rank-zero tensor (the time axis must exist)", Iir.apply, c, np.asarray(1.0, np.float32))
    raises("filtfilt: cannot analyse a rank-zero tensor (the time axis must exist)", Iir.filtfilt, c, np.asarray(1.0, np.float32))
    raises("apply: cannot start from a state of shape (2,) (zi must be [sections; 2] = (2, 2) or one per channel, (3, 2, 2))", Iir.apply, c, x, np.zeros(2))
    raises("apply: cannot start from a state of shape (4, 2, 2) (zi must be [sections; 2] = (2, 2) or one per channel, (3, 2, 2))", Iir.apply, c, x,
           np.zeros((4, 2, 2)))
    assert c.padlen == 15
    raises("filtfilt: cannot extend a signal of 15 samples by 15 on each side (n must exceed padlen = 15)", Iir.filtfilt, c, x[:, :15])
    raises("filtfilt: cannot extend a signal of 0 samples by 15 on each side (n must exceed padlen = 15)", Iir.filtfilt, c, np.zeros((0, 0), np.float32))


def test_device_float64_is_refused():
    """as energy.py words it; the check looks at the tensor alone, so a stand-in shows it without a device"""
    class Resident:
        device, bytes = True, 8
    for op in ("apply", "filtfilt", "step"):
        with pytest.raises(S.Failure) as e:
            Iir._refuse_device_float64(op, Resident())
        assert str(e.value) == "%s: device-resident float64 audio is not supported; pass a host array" % op


def test_empty_results_without_a_launch():
    c = Iir.Config.create(R.cascade(2))
    for dtype in (np.float32, np.float64):
        out = Iir.apply(c, np.ones((3, 0), dtype))
        assert out.shape == (3, 0) and out.dtype == dtype
        out, zf = Iir.apply(c, np.ones((2, 0, 7), dtype), return_state=True)
        assert out.shape == (2, 0, 7) and zf.shape == (2, 0, 2, 2) and zf.dtype == np.float64
        z = R.batch_state(1, 1, 2)[0]
        out, zf = Iir.apply(c, np.ones((3, 0), dtype), zi=z, return_state=True)
        assert out.shape == (3, 0) and np.array_equal(zf, np.broadcast_to(z, (3, 2, 2)))
        assert Iir.filtfilt(c, np.ones((0, 40), dtype)).shape == (0, 40)
    # the ABI's own empty signal hands the state back too, before it asks for a device
    z = np.ascontiguousarray(R.batch_state(2, 3, 2))
    zf = np.full((3, 2, 2), np.nan)
    assert _lib.lib.smx_iir_apply_f32(c._h, None, 3, 0, C.c_void_p(z.ctypes.data), 1, None, C.c_void_p(zf.ctypes.data)) == _lib.SMX_OK
    assert np.array_equal(zf, z)


def test_kernel_bookkeeping_on_shapes_alone():
    c = Iir.Config.create(R.cascade(2))
    raises("prepare: cannot keep the state of 0 channels (channels must be at least 1)", Iir.Kernel.prepare, c, 0)
    k = Iir.Kernel.prepare(c, 2, 5)
    assert k.lead_shape == (2, 5) and k.position == 0
    assert k.step(np.zeros((2, 5, 0), np.float32)) is None and k.position == 0
    raises("step: cannot analyse a rank-zero tensor (the time axis must exist)", k.step, np.asarray(1.0, np.float32))
    raises("step: cannot filter a chunk of leading shape (3,) with a kernel prepared for (2, 5)", k.step, np.zeros((3, 4), np.float32))
    assert k.flush() == [] and k.flush() == []
    raises(DRAINED, k.step, np.zeros((2, 5, 4), np.float32))
    raises(DRAINED, k.step, np.zeros((2, 5, 0), np.float32))
    k.reset()
    assert k.step(np.zeros((2, 5, 0), np.float32)) is None
    assert Iir.Kernel.prepare(c).lead_shape == () and Iir.Kernel.prepare(c, (4,)).lead_shape == (4,)


def test_the_abi_checks_before_it_asks_for_a_device():
    lib = _lib.lib
    c = Iir.Config.create(R.cascade(1))
    a = np.zeros(64, np.float32)
    ptr = C.c_void_p(a.ctypes.data)
    assert lib.smx_iir_filtfilt_card_f32(c._h, None, ptr, 1, 9, 9, ptr) == _lib.SMX_INVALID_ARGUMENT
    assert lib.smx_last_error().decode() == "filtfilt: cannot extend a signal of 9 samples by 9 on each side (n must exceed padlen = 9)"
    assert lib.smx_iir_apply_card_f32(c._h, None, ptr, 1, 64, 32, None, None, ptr, None) == _lib.SMX_FAILURE
    assert lib.smx_iir_apply_f32(None, ptr, 1, 64, None, 0, ptr, None) == _lib.SMX_FAILURE
    handle = C.c_void_p()
    assert lib.smx_iir_create(ptr, 0, C.byref(handle)) == _lib.SMX_INVALID_ARGUMENT


def test_header_naming_rules():
    """the device-tensor entries end in _card_f32 and take the stream directly behind the handle; no smx_iir_ declaration matches a
    pattern by which an older suite collects entries, and every declaration has its ctypes row with as many arguments"""
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "soundml_amd.h")).read(), flags=re.S)
    found = {}
    for m in re.finditer(r"\b(?:int|int64_t|void) (smx_iir_[a-z0-9_]*)\s*\(([^)]*)\)\s*;", header):
        found[m.group(1)] = [p.strip() for p in m.group(2).split(",")]
    assert len(found) == 23 and set(found) == {n for n in _lib.SIGNATURES if n.startswith("smx_iir_")}
    taken = re.compile(r"_dev$|_dev_f(32|64)$|_device_f32$|_resident_f32$|_hbm_f32$|_accel_f32$|_gpu_f32$|_vram_f32$")
    for name, params in found.items():
        assert not taken.search(name), name
        assert params[-1] != "void *stream", name
        args = _lib.SIGNATURES[name][1]
        assert len(args) == (0 if params == ["void"] else len(params)), name
        if name.endswith("_card_f32"):
            assert params[1] == "void *stream" and "int64_t x_stride" in params, name
        else:
            assert not any("stream" in p for p in params), name
    assert sorted(n for n in found if n.endswith("_card_f32")) == ["smx_iir_apply_card_f32", "smx_iir_filtfilt_card_f32", "smx_iir_kernel_step_card_f32"]
    assert not re.findall(r"\b(smx_iir_\w+)\s*\([^;{}]*?void\s*\*\s*stream\s*\)\s*;", header)
