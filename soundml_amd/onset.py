"""Spectral-flux onset strength on MI355X (reference: soundml/lib/onset.ml, re-exported flat as ``Soundml.onset_strength`` /
``onset_strength_stage``).

    env = onset_strength(stft_config, mel_config, x, lag=1)      # [...; n] -> [...; frames]
    stage = onset_strength_stage(lag=1)                          # log-spectral chunks [...; bins; frames] -> [...; frames]

The flat function: mel_spectrogram, float64 decibels under the whole tensor's 80 dB clamp, the mean over mels of the positive
part of db[., t] - db[., t - lag] (zero for t < lag), shifted right by fft_size / (2 hop) frames for centred analysis, one
rounding to the dtype of x.  The stage carries the last ``lag`` frames from chunk to chunk and applies neither clamp nor shift.
"""
from __future__ import annotations

import numpy as np

from . import _lib
from ._lib import check, lib
from ._tensor import OUT, STREAM, Batch, copy, is_torch, join, prod, refuse_device_float64
from . import stft as Stft


def onset_strength(stft_config, mel_config, x, lag: int = 1):
    """``Soundml.onset_strength stft mel ?lag x`` (onset.ml:153-199)."""
    lag = int(lag)
    # lag and the two fft sizes come before the tensor is looked at: let the ABI word them
    check(lib.smx_onset_strength_f32(stft_config._h, mel_config._h, None, 0, 0, lag, None))
    b = Batch(x, "onset_strength")
    n = int(b.shape[-1])
    lead_shape = b.shape[:-1]
    lead = prod(lead_shape)
    shape = lead_shape + (Stft.frames(stft_config, n),)
    refuse_device_float64("onset_strength", b)
    return b.run((lib.smx_onset_strength_f32, lib.smx_onset_strength_f64), (stft_config._h, mel_config._h, b.ptr(), lead, n, lag, OUT),
                 lib.smx_onset_strength_dev_f32, (stft_config._h, mel_config._h, b.ptr(), lead, n, n, lag, OUT, STREAM), shape)


def flux(s, lag: int = 1):
    """One chunk of the flux on its own (``state_step`` with an empty carry, onset.ml:82-122): decibels [...; bins; frames] ->
    [...; frames], zero for the first ``lag`` frames."""
    op = "onset_strength_stage"
    nd = len(s.shape)
    if nd < 2:
        check(lib.smx_onset_flux_f32(None, 1, 1, 0, int(lag), None))     # the lag comes first
        raise _lib.InvalidArgument("%s: cannot aggregate a rank-%d tensor (the onset flux needs [...; bins; frames])" % (op, nd))
    b = Batch(s, op)
    lead_shape, bins, frames = b.shape[:-2], int(b.shape[-2]), int(b.shape[-1])
    lead = prod(lead_shape)
    skip = lead == 0 or bins == 0 or frames == 0
    if skip:
        check(lib.smx_onset_flux_f32(None, lead, bins, frames, int(lag), None))
    else:
        refuse_device_float64(op, b, "spectrograms are")
    return b.run((lib.smx_onset_flux_f32, lib.smx_onset_flux_f64), (b.ptr(), lead, bins, frames, int(lag), OUT),
                 lib.smx_onset_flux_dev_f32, (b.ptr(), lead, bins, frames, int(lag), OUT, STREAM), lead_shape + (frames,),
                 skip=skip, empty="uninitialised")


class OnsetStrengthStage:
    """``Soundml.onset_strength_stage ?lag ()`` (onset.ml:126-149): one value per incoming frame, zeros for the first ``lag``
    frames of the stream; the last min(lag, seen) frames are carried, in the chunks' own container."""
    latency = 0

    def __init__(self, lag: int = 1):
        self.lag = int(lag)
        check(lib.smx_onset_flux_f32(None, 1, 1, 0, self.lag, None))     # onset.ml:29-34
        self._carry = None

    def step(self, chunk):
        if len(chunk.shape) < 2 or 0 in tuple(chunk.shape)[:-1] or int(chunk.shape[-1]) == 0:
            return flux(chunk, self.lag)                                  # the errors and the empty envelope: no state changes
        if self._carry is None:
            ext, keep = chunk, 0
        else:
            keep = int(self._carry.shape[-1])
            if is_torch(chunk):
                ext = join([self._carry.to(device=chunk.device, dtype=chunk.dtype), chunk])
            else:
                ext = join([self._carry, np.asarray(chunk)])
        out = flux(ext, self.lag)[..., keep:]
        held = min(self.lag, int(ext.shape[-1]))
        tail = ext[..., int(ext.shape[-1]) - held:]
        self._carry = copy(tail)
        return out.contiguous() if is_torch(out) else np.ascontiguousarray(out)

    __call__ = step

    def flush(self):
        return []

    def reset(self):
        self._carry = None


def onset_strength_stage(lag: int = 1):
    return OnsetStrengthStage(lag)
