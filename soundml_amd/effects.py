"""Time-scale and pitch modification by the phase vocoder on MI355X (reference: soundml/lib/effects.ml,
effects.mli:137-254, re-exported flat as ``Soundml.time_stretch`` etc.).

    z2 = Effects.phase_vocoder(c, Stft.transform(c, x), rate=1.25)         # [...; bins; frames] -> [...; bins; ceil(frames / rate)]
    y = Effects.time_stretch(c, x, rate=0.8, phase="locked")               # [...; n] -> [...; rint(n / rate)]
    y = Effects.pitch_shift(c, x, Effects.semitones(4))                    # [...; n] -> [...; n], a major third up
    num, den = Effects.semitones(-12)                                      # (1, 2)

``rate`` above 1 shortens, below 1 lengthens.  The vocoder's phases are a float64 recurrence in the reference's operation
order whatever the dtype of the spectrum and whatever ``set_interior`` says; the interior chooses the arithmetic of the
STFT and the ISTFT around it in ``time_stretch`` (under "float64", float32 audio is widened first, the spectra stay
complex128 between the three stages and the result is rounded once).  ``pitch_shift`` is ``time_stretch`` at ``den / num``
followed by ``Resample.apply`` from ``num`` to ``den`` and a cut or zero-extension to the input length.  DEVIATION:
``Resample.apply`` is float32 here, so float64 audio is stretched in float64 and converted in float32.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _lib
from .resample import Config as _ResampleConfig
from ._lib import check, lib
from ._tensor import OUT, STREAM, Batch, is_device, is_torch, out_ptr, prod, refuse_device_float64, torch

_PHASE = {"independent": 0, "locked": 1}
_RESAMPLERS = {}    # (num, den, quality) -> Resample.Config: its filter bank is uploaded once, and freeing one waits for the device


def _resampler(num, den, quality):
    """The resampler of a ratio, kept for the next call (a config built per call would upload its bank and free it again,
    which synchronises the device); an unhashable quality gets a config of its own."""
    try:
        key = (num, den, quality if isinstance(quality, str) else tuple(quality))
        hash(key)
    except TypeError:
        return _ResampleConfig.create(num, den, quality)
    config = _RESAMPLERS.get(key)
    if config is None:
        if len(_RESAMPLERS) >= 64:
            _RESAMPLERS.pop(next(iter(_RESAMPLERS)))
        config = _RESAMPLERS[key] = _ResampleConfig.create(num, den, quality)
    return config


def _g(v: float) -> str:
    v = float(v)
    if math.isnan(v):
        return "nan"
    if math.isinf(v):
        return "inf" if v > 0 else "-inf"
    return "%g" % v


def _check_rate(fn, rate):   # effects.ml:96-102
    rate = float(rate)
    if not (math.isfinite(rate) and rate > 0.0):
        raise _lib.InvalidArgument("%s: cannot stretch by a rate of %s (the rate must be finite and positive)" % (fn, _g(rate)))
    return rate


def _check_rank(fn, x):   # effects.ml:119-123
    if len(x.shape) < 1:
        raise _lib.InvalidArgument("%s: cannot process a rank-zero tensor (the time axis must exist)" % fn)


def _phase(fn, phase):
    if phase not in _PHASE:
        raise _lib.InvalidArgument("%s: cannot use phase %r (one of 'independent', 'locked')" % (fn, phase))
    return _PHASE[phase]


def out_frames(frames: int, rate: float) -> int:
    """``out_frames`` (effects.ml:90-92): the output frames of ``phase_vocoder``, ``ceil(frames / rate)``."""
    count = C.c_int64()
    check(lib.smx_phase_vocoder_frames(int(frames), float(rate), C.byref(count)))
    return count.value


def stretch_length(n: int, rate: float) -> int:
    """The output length of ``time_stretch`` (effects.ml:295): ``n / rate`` rounded to nearest, ties to even."""
    length = C.c_int64()
    check(lib.smx_time_stretch_length(int(n), float(rate), C.byref(length)))
    return length.value


def semitones(n: float, bins_per_octave: int = 12):
    """``Effects.semitones ?bins_per_octave n`` (effects.ml:345-386): ``2 ** (n / bins_per_octave)`` as the best rational
    ``(num, den)`` with neither term above 512: ``semitones(12) == (2, 1)``, ``semitones(4) == (349, 277)``."""
    num, den = C.c_int64(), C.c_int64()
    check(lib.smx_semitones(float(n), int(bins_per_octave), C.byref(num), C.byref(den)))
    return num.value, den.value


def phase_vocoder(c, z, rate: float, phase: str = "independent"):
    """``Effects.phase_vocoder ?phase c ~rate z`` (effects.ml:285-289): complex ``[...; bins; frames]`` as ``Stft.transform``
    returns it -> ``[...; bins; ceil(frames / rate)]`` in the dtype of ``z``.  Only ``fft_size`` and ``hop`` of ``c`` are
    read."""
    fn = "phase_vocoder"
    rate = _check_rate(fn, rate)
    shape = tuple(z.shape)
    if len(shape) < 2:   # effects.ml:104-110
        raise _lib.InvalidArgument("%s: cannot vocode a rank-%d tensor (the bin and frame axes must exist)" % (fn, len(shape)))
    lead, bins, frames = prod(shape[:-2]), int(shape[-2]), int(shape[-1])
    if bins != c.bins:   # effects.ml:111-117
        raise _lib.InvalidArgument("%s: cannot vocode %d frequency bins of a %d-point transform (the bin axis must hold "
                                   "fft_size / 2 + 1 = %d values)" % (fn, bins, c.fft_size, c.bins))
    mode = _phase(fn, phase)
    out_shape = shape[:-1] + (out_frames(frames, rate),)
    if is_device(z):
        if z.dtype not in (torch.complex64, torch.complex128):
            z = z.to(torch.complex64)
        zc = z.contiguous()
        out = torch.zeros(out_shape, dtype=zc.dtype, device=zc.device)
        dev_fn = lib.smx_phase_vocoder_c64_dev if zc.dtype == torch.complex64 else lib.smx_phase_vocoder_c128_dev
        with torch.cuda.device(zc.device):
            stream = C.c_void_p(torch.cuda.current_stream(zc.device).cuda_stream)
            ptr = lambda t: C.c_void_p(torch.view_as_real(t).data_ptr()) if t.numel() else None
            check(dev_fn(c._h, ptr(zc), lead, bins, frames, rate, mode, ptr(out), stream))
        return out
    was_torch = is_torch(z)
    a = z.detach().cpu().numpy() if was_torch else np.asarray(z)
    if a.dtype not in (np.complex64, np.complex128):
        a = a.astype(np.complex64 if a.dtype == np.float32 else np.complex128)
    a = np.ascontiguousarray(a)
    out = np.zeros(out_shape, a.dtype)
    host_fn = lib.smx_phase_vocoder_c128 if a.dtype == np.complex128 else lib.smx_phase_vocoder_c64
    check(host_fn(c._h, C.c_void_p(a.ctypes.data), lead, bins, frames, rate, mode, out_ptr(out)))
    return torch.from_numpy(out) if was_torch else out


def _signal_call(fn, x, out_len, host, device, args_before, args_after):
    b = Batch(x, fn)
    shape = b.shape
    refuse_device_float64(fn, b)
    args = (*args_before, b.ptr(), prod(shape[:-1]), int(shape[-1]), *args_after, OUT)
    return b.run(host, args, device, args + (STREAM,), shape[:-1] + (out_len,))


def time_stretch(c, x, rate: float, phase: str = "independent"):
    """``Effects.time_stretch ?phase c ~rate x`` (effects.ml:291-298): audio ``[...; n]`` -> ``[...; rint(n / rate)]`` in
    x's dtype; bit for bit ``Stft.invert(c, phase_vocoder(c, Stft.transform(c, x), rate), length=rint(n / rate))``, without
    the spectra leaving the device."""
    fn = "time_stretch"
    rate = _check_rate(fn, rate)
    _check_rank(fn, x)
    mode = _phase(fn, phase)
    length = stretch_length(int(x.shape[-1]), rate)
    return _signal_call(fn, x, length, (lib.smx_time_stretch_f32, lib.smx_time_stretch_f64), lib.smx_time_stretch_f32_dev,
                        (c._h,), (rate, mode))


def pitch_shift(c, x, ratio, phase: str = "independent", quality="high"):
    """``Effects.pitch_shift ?phase ?quality c ~ratio x`` (effects.ml:324-334): audio ``[...; n]`` -> ``[...; n]`` with every
    frequency multiplied by ``num / den`` (``ratio = (num, den)``; ``semitones`` names the ratios of equal temperament).
    ``quality`` is the resampler's (``Resample.Config.create``), whose conditions raise from there."""
    fn = "pitch_shift"
    num, den = (int(t) for t in ratio)
    if num < 1 or den < 1:   # effects.ml:316-322
        raise _lib.InvalidArgument("%s: cannot shift by a frequency ratio of %d/%d (both terms must be at least 1)" % (fn, num, den))
    _check_rank(fn, x)
    mode = _phase(fn, phase)
    # time_stretch's conditions (Stft.invert's among them) come before the resampler's, as in the reference: the checks alone, no clip
    check(lib.smx_time_stretch_f32(c._h, None, 0, int(x.shape[-1]), float(den) / float(num), mode, None))
    resampler = _resampler(num, den, quality)
    return _signal_call(fn, x, int(x.shape[-1]), (lib.smx_pitch_shift_f32, lib.smx_pitch_shift_f64), lib.smx_pitch_shift_f32_dev,
                        (c._h, resampler._h, mode), ())
