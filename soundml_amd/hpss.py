"""Harmonic/percussive separation on MI355X (reference: soundml/lib/hpss.ml, re-exported flat as
``Soundml.hpss`` etc., soundml.ml:160-173).

    mask_h, mask_p = Hpss.hpss_masks(s, kernel_size=(31, 31), power=2.0, margin=(1.0, 1.0))   # [...; bins; frames]
    h, p = Hpss.hpss_of_spectrogram(s)             # s * mask_h, s * mask_p
    z_h, z_p = Hpss.hpss_of_stft(Stft.transform(c, x))
    y_h, y_p = Hpss.hpss(c, x)                     # transform -> hpss_of_stft -> invert(length=n), on the device
    y_h = Hpss.harmonic(c, x); y_p = Hpss.percussive(c, x)

Two running medians (``kernel_size = (frames, bins)``) select values of the magnitude plane, a pair of masks
(Wiener-like for finite ``power``, hard for ``power=float("inf")``) shares it out.  Any kernel size of at least 1
is legal; the default 31 x 31 on large float32 planes has a kernel of its own.  NaN inputs give unspecified
results, as in the reference.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _lib
from ._lib import check, lib
from ._tensor import OUT, STREAM, Batch, is_device, is_torch, out_ptr, prod, refuse_device_float64, torch

DEFAULT_KERNEL = (31, 31)
DEFAULT_MARGIN = (1.0, 1.0)


def _g(v: float) -> str:
    v = float(v)
    if math.isnan(v):
        return "nan"
    if math.isinf(v):
        return "inf" if v > 0 else "-inf"
    return "%g" % v


def _validate(fn, kernel_size, power, margin):
    """check_kernel, check_power, check_margin (hpss.ml:373-396), in the reference's order and words."""
    k_h, k_p = (int(k) for k in kernel_size)
    m_h, m_p = (float(m) for m in margin)
    power = float(power)
    if k_h < 1 or k_p < 1:
        raise _lib.InvalidArgument(
            "%s: cannot median-filter with a kernel of (%d, %d) (both kernel sizes must be at least 1)" % (fn, k_h, k_p))
    if math.isnan(power) or power <= 0.0:
        raise _lib.InvalidArgument(
            "%s: cannot raise the mask to the power %s (power must be strictly positive, or infinite for a hard mask)"
            % (fn, _g(power)))
    if not (math.isfinite(m_h) and math.isfinite(m_p) and m_h >= 1.0 and m_p >= 1.0):
        raise _lib.InvalidArgument(
            "%s: cannot bias the decision by a margin of (%s, %s) (both margins must be finite and at least 1)"
            % (fn, _g(m_h), _g(m_p)))
    return (k_h, k_p, power, m_h, m_p)


def _check_rank(fn, nd):   # hpss.ml:365-371
    if nd < 2:
        raise _lib.InvalidArgument(
            "%s: cannot separate a rank-%d tensor (a spectrogram carries a bin axis and a frame axis)" % (fn, nd))


def _dtype_name(x):
    return str(x.dtype).replace("torch.", "")


def _check_real_dtype(fn, x):   # hpss.ml:351-363
    name = _dtype_name(x)
    if name not in ("float32", "float64"):
        raise _lib.InvalidArgument(
            "%s: cannot separate %s spectra (the median kernel carries float32 and float64)" % (fn, name))


def _planes(fn, s, params, host, device):
    _check_rank(fn, len(s.shape))
    _check_real_dtype(fn, s)
    b = Batch(s, fn)
    shape = b.shape
    refuse_device_float64(fn, b, "spectrograms are")
    args = (b.ptr(), prod(shape[:-2]), int(shape[-2]), int(shape[-1]), *params, OUT, OUT)
    return b.run(host, args, device, args + (STREAM,), [shape, shape])


def hpss_masks(s, kernel_size=DEFAULT_KERNEL, power: float = 2.0, margin=DEFAULT_MARGIN):
    """``Hpss.hpss_masks ?kernel_size ?power ?margin s`` (hpss.ml:411-414): the harmonic and percussive masks."""
    fn = "hpss_masks"
    params = _validate(fn, kernel_size, power, margin)
    return _planes(fn, s, params, (lib.smx_hpss_masks_f32, lib.smx_hpss_masks_f64), lib.smx_hpss_masks_f32_dev)


def hpss_of_spectrogram(s, kernel_size=DEFAULT_KERNEL, power: float = 2.0, margin=DEFAULT_MARGIN):
    """``Hpss.hpss_of_spectrogram`` (hpss.ml:416-420): ``(s * mask_h, s * mask_p)``."""
    fn = "hpss_of_spectrogram"
    params = _validate(fn, kernel_size, power, margin)
    return _planes(fn, s, params, (lib.smx_hpss_of_spectrogram_f32, lib.smx_hpss_of_spectrogram_f64),
                   lib.smx_hpss_of_spectrogram_f32_dev)


def hpss_of_stft(z, kernel_size=DEFAULT_KERNEL, power: float = 2.0, margin=DEFAULT_MARGIN):
    """``Hpss.hpss_of_stft`` (hpss.ml:436-459): complex [...; bins; frames] as ``Stft.transform`` returns it ->
    the two complex components, magnitudes masked and phases kept."""
    fn = "hpss_of_stft"
    params = _validate(fn, kernel_size, power, margin)
    shape = tuple(z.shape)
    _check_rank(fn, len(shape))
    lead, bins, frames = prod(shape[:-2]), int(shape[-2]), int(shape[-1])
    if is_device(z):
        if z.dtype not in (torch.complex64, torch.complex128):
            z = z.to(torch.complex64)
        if z.dtype != torch.complex64:
            raise _lib.Failure("%s: device-resident complex128 spectra are not supported; pass a host array" % fn)
        zc = z.contiguous()
        z_h, z_p = torch.zeros_like(zc), torch.zeros_like(zc)
        with torch.cuda.device(zc.device):
            stream = C.c_void_p(torch.cuda.current_stream(zc.device).cuda_stream)
            ptr = lambda t: C.c_void_p(torch.view_as_real(t).data_ptr())
            check(lib.smx_hpss_of_stft_c64_dev(ptr(zc), lead, bins, frames, *params, ptr(z_h), ptr(z_p), stream))
        return z_h, z_p
    was_torch = is_torch(z)
    a = z.detach().cpu().numpy() if was_torch else np.asarray(z)
    if a.dtype not in (np.complex64, np.complex128):
        a = a.astype(np.complex64 if a.dtype == np.float32 else np.complex128)
    a = np.ascontiguousarray(a)
    z_h, z_p = np.zeros(shape, a.dtype), np.zeros(shape, a.dtype)
    host_fn = lib.smx_hpss_of_stft_c128 if a.dtype == np.complex128 else lib.smx_hpss_of_stft_c64
    check(host_fn(C.c_void_p(a.ctypes.data), lead, bins, frames, *params, out_ptr(z_h), out_ptr(z_p)))
    if was_torch:
        return torch.from_numpy(z_h), torch.from_numpy(z_p)
    return z_h, z_p


def _separate(fn, c, x, kernel_size, power, margin, want_h, want_p):
    """``separate`` (hpss.ml:477-492): kernel, power, margin, rank, dtype; then the round trip inside the library."""
    params = _validate(fn, kernel_size, power, margin)
    if len(x.shape) < 1:
        raise _lib.InvalidArgument("%s: cannot separate a rank-zero tensor (the time axis must exist)" % fn)
    _check_real_dtype(fn, x)
    b = Batch(x, fn)
    shape = b.shape
    lead, n = prod(shape[:-1]), int(shape[-1])
    refuse_device_float64(fn, b)
    args = (c._h, b.ptr(), lead, n, *params, OUT, OUT)
    return b.run((lib.smx_hpss_f32, lib.smx_hpss_f64), args, lib.smx_hpss_f32_dev, args + (STREAM,),
                 [shape if want_h else None, shape if want_p else None], prefill=True)


def hpss(c, x, kernel_size=DEFAULT_KERNEL, power: float = 2.0, margin=DEFAULT_MARGIN):
    """``Hpss.hpss c ?kernel_size ?power ?margin x`` (hpss.ml:494-496): audio [...; n] -> (harmonic, percussive),
    each [...; n] in x's dtype; bit for bit ``Stft.invert(c, ., length=n)`` of the halves of
    ``hpss_of_stft(Stft.transform(c, x))``, without the spectra leaving the device."""
    return _separate("hpss", c, x, kernel_size, power, margin, True, True)


def harmonic(c, x, kernel_size=DEFAULT_KERNEL, power: float = 2.0, margin=DEFAULT_MARGIN):
    """``Hpss.harmonic`` (hpss.ml:498-500): the first component of ``hpss`` (the other inversion is skipped)."""
    return _separate("harmonic", c, x, kernel_size, power, margin, True, False)[0]


def percussive(c, x, kernel_size=DEFAULT_KERNEL, power: float = 2.0, margin=DEFAULT_MARGIN):
    """``Hpss.percussive`` (hpss.ml:502-504): the second component of ``hpss``."""
    return _separate("percussive", c, x, kernel_size, power, margin, False, True)[1]
