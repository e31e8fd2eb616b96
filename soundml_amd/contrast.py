"""Octave-band spectral contrast on MI355X (reference: soundml/lib/contrast.ml, re-exported flat as
``Soundml.spectral_contrast`` / ``spectral_contrast_of_spectrogram`` / ``spectral_contrast_stage``).

    c = spectral_contrast(stft_config, x, sample_rate=22050)              # [...; n] -> [...; n_bands + 1; frames]
    c = spectral_contrast_of_spectrogram(s, sample_rate=22050)            # [...; bins; frames] magnitudes
    stage = spectral_contrast_stage(stft_config, sample_rate=22050)       # per chunk, no whole-signal clamp

Per band and frame: the mean of the ``take`` largest magnitudes against the mean of the ``take`` smallest, an exact selection
with float64 means, as a difference (``linear``) or a difference of decibels; the flat functions clamp each side 80 dB under
the maximum of its whole tensor.  One rounding to the dtype of the input.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import check, lib
from ._tensor import OUT, STREAM, Batch, Stateless, prod, refuse_device_float64
from . import stft as Stft


def plan(n_bands: int, f_min: float, quantile: float, sample_rate: int, fft_size: int):
    """The band plan of contrast.ml:60-142 as a list of (first bin, bins, take), n_bands + 1 entries (host integers only)."""
    rows = max(int(n_bands), 0) + 1
    lo, sub_len, take = (np.zeros(rows, np.int64) for _ in range(3))
    check(lib.smx_spectral_contrast_plan(int(n_bands), float(f_min), float(quantile), int(sample_rate), int(fft_size),
                                         C.c_void_p(lo.ctypes.data), C.c_void_p(sub_len.ctypes.data), C.c_void_p(take.ctypes.data)))
    return [(int(a), int(b), int(c)) for a, b, c in zip(lo, sub_len, take)]


def _params(n_bands, f_min, quantile, linear, sample_rate):
    return int(n_bands), float(f_min), float(quantile), 1 if linear else 0, int(sample_rate)


def spectral_contrast(stft_config, x, sample_rate: int, n_bands: int = 6, f_min: float = 200.0, quantile: float = 0.02,
                      linear: bool = False):
    """``Soundml.spectral_contrast stft ?n_bands ?f_min ?quantile ?linear ~sample_rate x`` (contrast.ml:208-218)."""
    q = _params(n_bands, f_min, quantile, linear, sample_rate)
    # the plan's checks come before the tensor is looked at: let the ABI word them
    check(lib.smx_spectral_contrast_f32(stft_config._h, None, 0, 0, *q, None))
    b = Batch(x, "spectral_contrast")
    n = int(b.shape[-1])
    lead_shape = b.shape[:-1]
    lead = prod(lead_shape)
    shape = lead_shape + (q[0] + 1, Stft.frames(stft_config, n))
    refuse_device_float64("spectral_contrast", b)
    return b.run((lib.smx_spectral_contrast_f32, lib.smx_spectral_contrast_f64), (stft_config._h, b.ptr(), lead, n, *q, OUT),
                 lib.smx_spectral_contrast_dev_f32, (stft_config._h, b.ptr(), lead, n, n, *q, OUT, STREAM), shape)


def _of_spectrogram(op, s, fft_size, q, clamped):
    nd = len(s.shape)
    if nd < 2:   # contrast.ml:157-162, 226-232
        raise _lib.InvalidArgument("%s: cannot analyse a rank-%d tensor (spectral contrast needs [...; bins; frames])" % (op, nd))
    b = Batch(s, op)
    lead_shape, bins, frames = b.shape[:-2], int(b.shape[-2]), int(b.shape[-1])
    lead = prod(lead_shape)
    args = (lead, bins, frames, fft_size) + q + (1 if clamped else 0,)
    # what does not read the data, worded by the ABI before anything is allocated (no clips: no device work)
    check(lib.smx_spectral_contrast_of_spectrogram_f32(None, 0, bins, 0, *args[3:], None))
    skip = lead == 0 or bins == 0 or frames == 0
    if not skip:
        refuse_device_float64(op, b, "spectrograms are")
    return b.run((lib.smx_spectral_contrast_of_spectrogram_f32, lib.smx_spectral_contrast_of_spectrogram_f64), (b.ptr(), *args, OUT),
                 lib.smx_spectral_contrast_of_spectrogram_dev_f32, (b.ptr(), *args, OUT, STREAM), lead_shape + (q[0] + 1, frames),
                 skip=skip, empty="uninitialised")


def spectral_contrast_of_spectrogram(s, sample_rate: int, n_bands: int = 6, f_min: float = 200.0, quantile: float = 0.02,
                                     linear: bool = False):
    """``Soundml.spectral_contrast_of_spectrogram ?n_bands ?f_min ?quantile ?linear ~sample_rate s`` (contrast.ml:223-252):
    the FFT size is the one the bin count implies; the magnitudes must be non-negative."""
    return _of_spectrogram("spectral_contrast_of_spectrogram", s, 0, _params(n_bands, f_min, quantile, linear, sample_rate), True)


def spectral_contrast_stage(stft_config, sample_rate: int, n_bands: int = 6, f_min: float = 200.0, quantile: float = 0.02,
                            linear: bool = False):
    """``Soundml.spectral_contrast_stage`` (contrast.ml:254-261): a memoryless stage over magnitude chunks [...; bins; frames].
    The parameters are checked here, where the stage is built; the 80 dB clamp of the flat functions is a whole-signal
    reduction and is left out."""
    q = _params(n_bands, f_min, quantile, linear, sample_rate)
    fft_size = int(stft_config.fft_size)
    check(lib.smx_spectral_contrast_of_spectrogram_f32(None, 0, fft_size // 2 + 1, 0, fft_size, *q, 0, None))
    return Stateless(lambda s: _of_spectrogram("spectral_contrast_stage", s, fft_size, q, False))
