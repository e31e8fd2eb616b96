"""Recursive filters as cascaded second-order sections on MI355X (scipy.signal's ``sosfilt`` / ``sosfilt_zi`` / ``sosfiltfilt``;
the reference lists "IIR/FIR filtering" as planned, README.md:27-34, and has no such module).

    c = Iir.Config.create(sos)                          # [S; 6] float64 rows b0 b1 b2 a0 a1 a2, a0 == 1, S <= Iir.MAX_SECTIONS
    y = Iir.apply(c, x)                                 # [...; n] -> [...; n]
    y, zf = Iir.apply(c, x, zi=zi, return_state=True)   # zi [S; 2] or [...; S; 2] float64; zf [...; S; 2]
    y = Iir.filtfilt(c, x)                              # zero phase: sosfiltfilt with its defaults
    zi = Iir.zi(c)                                      # the unit-step steady state, [S; 2]
    k = Iir.Kernel.prepare(c, channels)                 # k.step(chunk) -> [...; m] | None; k.flush() -> []; k.reset()

There is no filter designer: the coefficients are the caller's, e.g. ``scipy.signal.butter(..., output="sos")``.  Float64 inside,
one rounding to the dtype of the input.  The time axis is cut into blocks of ``Iir.BLOCK`` samples whose entering states follow
from one another by one stated sum, so both kernels, a leading slice of a batch and every chunking of a
``Kernel`` give the same bits.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import check, lib
from ._tensor import OUT, STREAM, Batch, is_device, is_torch, out_ptr, prod, refuse_device_float64, torch

BLOCK = int(lib.smx_iir_block())
SPAN_BLOCKS = int(lib.smx_iir_span_blocks())
MAX_SECTIONS = int(lib.smx_iir_max_sections())


class Config:
    def __init__(self, handle, sos):
        self._h, self.sos, self.sections = handle, sos, int(sos.shape[0])

    @staticmethod
    def create(sos) -> "Config":
        sos = np.ascontiguousarray(np.asarray(sos, dtype=np.float64))
        if sos.ndim != 2 or sos.shape[1] != 6:
            raise _lib.InvalidArgument("create: cannot read an array of shape %s as second-order sections (sos must be [sections; 6])"
                                       % (tuple(sos.shape),))
        handle = C.c_void_p()
        check(lib.smx_iir_create(C.c_void_p(sos.ctypes.data), int(sos.shape[0]), C.byref(handle)))
        return Config(handle, sos)

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h and lib is not None:
            try:
                lib.smx_iir_destroy(h)
            except Exception:
                pass

    padlen = property(lambda self: int(lib.smx_iir_padlen(self._h)))

    @property
    def matrix(self) -> np.ndarray:
        """M [2S; 2S]: column i is the end state of ``BLOCK`` zero-input steps of the cascade from the unit state e_i."""
        m = np.empty((2 * self.sections, 2 * self.sections), np.float64)
        check(lib.smx_iir_matrix(self._h, C.c_void_p(m.ctypes.data)))
        return m


def zi(c: Config) -> np.ndarray:
    """The state of the cascade settled on a unit step (``sosfilt_zi`` in closed form), [S; 2] float64."""
    out = np.empty((c.sections, 2), np.float64)
    check(lib.smx_iir_zi(c._h, C.c_void_p(out.ctypes.data)))
    return out


_refuse_device_float64 = refuse_device_float64


def _state(c, zi_, lead_shape):
    """-> (float64 array or None, one row per channel?)"""
    if zi_ is None:
        return None, False
    if is_device(zi_) and tuple(zi_.shape) == tuple(lead_shape) + (c.sections, 2) and len(lead_shape) > 0:
        return zi_.to(torch.float64).contiguous(), True      # one state per channel, already resident: no copy, no wait
    z = zi_.detach().cpu().numpy() if is_torch(zi_) else np.asarray(zi_)
    z = np.ascontiguousarray(z, dtype=np.float64)
    if z.shape == (c.sections, 2):
        return z, False
    if z.shape == tuple(lead_shape) + (c.sections, 2):
        return z, True
    raise _lib.InvalidArgument("apply: cannot start from a state of shape %s (zi must be [sections; 2] = %s or one per channel, %s)"
                               % (tuple(z.shape), (c.sections, 2), tuple(lead_shape) + (c.sections, 2)))


def apply(c: Config, x, zi=None, return_state: bool = False):
    """``sosfilt(sos, x, zi=zi)`` along the last axis: [...; n] -> [...; n] (and the final state [...; S; 2] float64)."""
    b = Batch(x, "apply")
    _refuse_device_float64("apply", b)
    n, lead_shape = int(b.shape[-1]), b.shape[:-1]
    lead = prod(lead_shape)
    z, rows = _state(c, zi, lead_shape)
    state_shape = tuple(lead_shape) + (c.sections, 2)
    if lead == 0 or n == 0:                              # nothing to filter: no launch, the state given is the state returned
        out = b.wrap(b.empty(b.shape))
        if not return_state:
            return out
        zf = np.zeros(state_shape) if z is None else np.ascontiguousarray(np.broadcast_to(z.cpu().numpy() if is_torch(z) else z, state_shape))
        if b.device:
                return out, torch.from_numpy(zf).to(b.data.device)
        return out, b.wrap(zf)
    if is_torch(z) and not b.device:
        z = z.cpu().numpy()
    zp = C.c_void_p(z.ctypes.data) if z is not None and not is_torch(z) else None
    d_rows = zf = None                                   # the float64 states lie on the signal's side
    if b.device:
        if return_state:
            zf = torch.empty(state_shape, dtype=torch.float64, device=b.data.device)
        if rows:
            d_rows = z if is_torch(z) else torch.from_numpy(z).to(b.data.device)
    elif return_state:
        zf = np.zeros(state_shape)
    ptr = lambda t: None if t is None else out_ptr(t)
    out = b.run((lib.smx_iir_apply_f32, lib.smx_iir_apply_f64), (c._h, b.ptr(), lead, n, zp, 1 if rows else 0, OUT, ptr(zf)),
                lib.smx_iir_apply_card_f32, (c._h, STREAM, b.ptr(), lead, n, n, None if rows else zp, ptr(d_rows), OUT, ptr(zf)),
                b.shape, overwritten=True)
    if d_rows is not None:
        d_rows.record_stream(torch.cuda.current_stream(b.data.device))
    return (out, b.wrap(zf)) if return_state else out


def filtfilt(c: Config, x):
    """``sosfiltfilt(sos, x)`` along the last axis with scipy's defaults (odd extension by ``c.padlen`` samples): [...; n] -> [...; n]."""
    b = Batch(x, "filtfilt")
    _refuse_device_float64("filtfilt", b)
    n, lead_shape = int(b.shape[-1]), b.shape[:-1]
    lead = prod(lead_shape)
    check(lib.smx_iir_filtfilt_f32(c._h, None, 0, n, None))          # the section at a pole, then the length, worded by the ABI
    return b.run((lib.smx_iir_filtfilt_f32, lib.smx_iir_filtfilt_f64), (c._h, b.ptr(), lead, n, OUT),
                 lib.smx_iir_filtfilt_card_f32, (c._h, STREAM, b.ptr(), lead, n, n, OUT), b.shape,
                 skip=lead == 0, empty="uninitialised", overwritten=True)


class Kernel:
    """The streaming form: the state of every channel stays on the device (6 S doubles each: the state entering the current block,
    the partial zero-state run, the running state); the position inside the block is a host integer.  ``step`` returns as many
    samples as it is given (latency zero); the concatenated steps equal ``apply`` of the whole signal bit for bit under every
    chunking.  Only shapes decide the control flow: device chunks cause no synchronisation."""
    latency = 0
    rate = (1, 1)

    def __init__(self, handle, config, lead_shape):
        self._h, self.config, self.lead_shape = handle, config, tuple(lead_shape)

    @staticmethod
    def prepare(c: Config, *lead_shape) -> "Kernel":
        if len(lead_shape) == 1 and isinstance(lead_shape[0], (tuple, list)):
            lead_shape = tuple(lead_shape[0])
        lead_shape = tuple(int(d) for d in lead_shape)
        handle = C.c_void_p()
        check(lib.smx_iir_kernel_prepare(c._h, prod(lead_shape), C.byref(handle)))
        return Kernel(handle, c, lead_shape)

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h and lib is not None:
            try:
                lib.smx_iir_kernel_destroy(h)
            except Exception:
                pass

    position = property(lambda self: int(lib.smx_iir_kernel_position(self._h)))

    def reset(self):
        check(lib.smx_iir_kernel_reset(self._h))

    def step(self, chunk):
        shape = tuple(chunk.shape)
        if len(shape) < 1:
            raise _lib.InvalidArgument("step: cannot analyse a rank-zero tensor (the time axis must exist)")
        m = int(shape[-1])
        if m == 0:
            check(lib.smx_iir_kernel_step_f32(self._h, None, 0, None))     # a drained kernel refuses an empty chunk too
            return None
        if shape[:-1] != self.lead_shape:
            raise _lib.InvalidArgument("step: cannot filter a chunk of leading shape %s with a kernel prepared for %s"
                                       % (shape[:-1], self.lead_shape))
        b = Batch(chunk, "step")
        _refuse_device_float64("step", b)
        return b.run((lib.smx_iir_kernel_step_f32, lib.smx_iir_kernel_step_f64), (self._h, b.ptr(), m, OUT),
                     lib.smx_iir_kernel_step_card_f32, (self._h, STREAM, b.ptr(), m, m, OUT), b.shape, overwritten=True)

    __call__ = step

    def flush(self):
        check(lib.smx_iir_kernel_flush(self._h))
        return []
