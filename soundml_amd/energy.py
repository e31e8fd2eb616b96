"""Frame energy features on MI355X (reference: soundml/lib/energy.ml, re-exported flat as ``Soundml.rms`` /
``rms_of_spectrogram`` / ``rms_stage`` / ``zero_crossing_rate`` / ``zero_crossing_rate_stage``).

    e = rms(x)                                       # [...; n] -> [...; 1; frames]
    z = zero_crossing_rate(x, threshold=1e-10)       # [...; n] -> [...; 1; frames]
    e = rms_of_spectrogram(s, frame_length=2048)     # magnitudes [...; bins; frames] -> [...; 1; frames]
    stage = rms_stage()                              # audio chunks [...; m] -> [...; 1; k] | None; flush() -> list

The signal is centred by ``frame_length // 2`` positions on each side (zeros for rms, copies of the first / last sample for the
zero-crossing rate) and frames advance by ``hop``; the borders are virtual, no padded copy is made.  Float64 inside, one rounding
to the dtype of the input.  A frame's sum of squares has one summation order, a function of its own samples, so a
leading slice of a batch and any chunking of a stage give the flat call's values bit for bit.
"""
from __future__ import annotations

import numpy as np

from . import _lib
from ._lib import check, lib
from ._tensor import Batch, is_torch, out_ptr, prod

RMS, ZCR = 0, 1
_NAMES = {RMS: "rms", ZCR: "zero_crossing_rate"}


def frames(n: int, frame_length: int = 2048, hop: int = 512) -> int:
    """The frame count of a length-``n`` signal (energy.ml:114-118): none for an empty one."""
    n, frame_length, hop = int(n), int(frame_length), int(hop)
    if n == 0:
        return 0
    padded = n + 2 * (frame_length // 2)
    return 0 if padded < frame_length else 1 + (padded - frame_length) // hop


def _zeros(b, shape):
    if b.device:
        import torch
        return torch.zeros(shape, dtype=b.data.dtype, device=b.data.device)
    return b.wrap(np.zeros(shape, dtype=b.data.dtype))


def _refuse_device_float64(op, b, what="audio is"):
    if b.device and b.bytes != 4:
        raise _lib.Failure("%s: device-resident float64 %s not supported; pass a host array" % (op, what))


def _centred(op, x, frame_length, hop, threshold):
    name = _NAMES[op]
    fl, hop, threshold = int(frame_length), int(hop), float(threshold)
    # the parameters come before the tensor is looked at: let the ABI word them
    if op == RMS:
        check(lib.smx_rms_f32(None, 0, 0, fl, hop, None))
    else:
        check(lib.smx_zero_crossing_rate_f32(None, 0, 0, fl, hop, threshold, None))
    b = Batch(x, name)
    _refuse_device_float64(name, b)
    n = int(b.shape[-1])
    lead_shape = b.shape[:-1]
    lead = prod(lead_shape)
    count = frames(n, fl, hop)
    if lead == 0 or count == 0:                          # energy.ml:354-366 `frameless`: zeros, no launch
        return _zeros(b, lead_shape + (1, count))
    out = b.empty(lead_shape + (1, count))
    if b.device:
        with b.device_guard():
            if op == RMS:
                check(lib.smx_rms_device_f32(b.ptr(), lead, n, n, fl, hop, out_ptr(out), b.stream()))
            else:
                check(lib.smx_zero_crossing_rate_device_f32(b.ptr(), lead, n, n, fl, hop, threshold, out_ptr(out), b.stream()))
        return out
    if op == RMS:
        fn = lib.smx_rms_f32 if b.bytes == 4 else lib.smx_rms_f64
        check(fn(b.ptr(), lead, n, fl, hop, out_ptr(out)))
    else:
        fn = lib.smx_zero_crossing_rate_f32 if b.bytes == 4 else lib.smx_zero_crossing_rate_f64
        check(fn(b.ptr(), lead, n, fl, hop, threshold, out_ptr(out)))
    return b.wrap(out)


def rms(x, frame_length: int = 2048, hop: int = 512):
    """``Soundml.rms ?frame_length ?hop x`` (energy.ml:380-381): sqrt(mean(x^2)) per frame, zero borders."""
    return _centred(RMS, x, frame_length, hop, 0.0)


def zero_crossing_rate(x, frame_length: int = 2048, hop: int = 512, threshold: float = 1e-10):
    """``Soundml.zero_crossing_rate ?frame_length ?hop ?threshold x`` (energy.ml:383-388): the fraction of consecutive samples of
    a frame that change sign, a sample being negative iff it lies strictly below ``-threshold``; edge borders."""
    return _centred(ZCR, x, frame_length, hop, threshold)


def rms_of_spectrogram(s, frame_length: int = 2048):
    """``Soundml.rms_of_spectrogram ?frame_length s`` (energy.ml:394-421): the frame energy of a magnitude spectrogram
    [...; frame_length // 2 + 1; frames] by Parseval's identity for the one-sided layout."""
    op = "rms_of_spectrogram"
    fl = int(frame_length)
    check(lib.smx_rms_of_spectrogram_f32(None, 0, max(fl, 0) // 2 + 1, 0, fl, None))      # the frame length comes first
    nd = len(s.shape)
    if nd < 2:
        raise _lib.InvalidArgument("%s: cannot analyse a rank-%d tensor (the spectrogram path needs [...; bins; frames])" % (op, nd))
    b = Batch(s, op)
    lead_shape, bins, count = b.shape[:-2], int(b.shape[-2]), int(b.shape[-1])
    lead = prod(lead_shape)
    check(lib.smx_rms_of_spectrogram_f32(None, 0, bins, 0, fl, None))                      # then the bin count
    _refuse_device_float64(op, b, "spectrograms are")
    if lead == 0 or count == 0:
        return _zeros(b, lead_shape + (1, count))
    out = b.empty(lead_shape + (1, count))
    if b.device:
        with b.device_guard():
            check(lib.smx_rms_of_spectrogram_device_f32(b.ptr(), lead, bins, count, fl, out_ptr(out), b.stream()))
        return out
    fn = lib.smx_rms_of_spectrogram_f32 if b.bytes == 4 else lib.smx_rms_of_spectrogram_f64
    check(fn(b.ptr(), lead, bins, count, fl, out_ptr(out)))
    return b.wrap(out)


def segment_frames(op: int, samples, count: int, frame_length: int, hop: int, threshold: float = 0.0):
    """Frames [0, count) of a segment of the padded stream, no border (energy.ml:157-183 `analyse`): the stages' body.
    [...; n] -> [...; 1; count]; (count - 1) * hop + frame_length <= n."""
    name = _NAMES[op] + "_stage"
    b = Batch(samples, name)
    _refuse_device_float64(name, b)
    n = int(b.shape[-1])
    lead_shape = b.shape[:-1]
    lead = prod(lead_shape)
    args = (int(op), float(threshold), int(frame_length), int(hop))
    if lead == 0 or int(count) == 0:
        check(lib.smx_energy_frames_f32(*args, None, lead, n, int(count), None))
        return _zeros(b, lead_shape + (1, int(count)))
    out = b.empty(lead_shape + (1, int(count)))
    if b.device:
        with b.device_guard():
            check(lib.smx_energy_frames_device_f32(*args, b.ptr(), lead, n, n, int(count), out_ptr(out), b.stream()))
        return out
    fn = lib.smx_energy_frames_f32 if b.bytes == 4 else lib.smx_energy_frames_f64
    check(fn(*args, b.ptr(), lead, n, int(count), out_ptr(out)))
    return b.wrap(out)


def _length(t) -> int:
    return int(t.shape[-1])


def _copy(t):
    return t.clone() if is_torch(t) else np.array(t)


def _join(parts):
    if is_torch(parts[0]):
        import torch
        return torch.cat(parts, dim=-1)
    return np.concatenate(parts, axis=-1)


def _zeros_like_lead(t, width):
    shape = tuple(t.shape[:-1]) + (width,)
    if is_torch(t):
        import torch
        return torch.zeros(shape, dtype=t.dtype, device=t.device)
    return np.zeros(shape, dtype=t.dtype)


def _repeat(sample, width):
    """[...; 1] -> [...; width] copies"""
    if is_torch(sample):
        return sample.expand(tuple(sample.shape[:-1]) + (width,)).contiguous()
    return np.repeat(sample, width, axis=-1)


class EnergyStage:
    """The streaming carry of energy.ml:194-347 behind ``rms_stage`` / ``zero_crossing_rate_stage``: the pending suffix of the
    padded stream (in the chunks' own container: numpy, or torch on the chunk's device), the last raw sample, and how many padded
    positions are still to drop when the hop outruns the data.  The left border installs with the first non-empty chunk, ``flush``
    appends the right one; every call frames ``pending ++ chunk`` for exactly the frames that became complete.  Only shapes
    decide the control flow: device chunks cause no synchronisation."""

    def __init__(self, op: int, frame_length: int = 2048, hop: int = 512, threshold: float = 0.0):
        self.op, self.frame_length, self.hop, self.threshold = int(op), int(frame_length), int(hop), float(threshold)
        # energy.ml:514-525: frame_length, hop, then the threshold, worded by the ABI
        check(lib.smx_energy_frames_f32(self.op, self.threshold, self.frame_length, self.hop, None, 0, 0, 0, None))
        self.name = _NAMES[self.op] + "_stage"
        self.border = self.frame_length // 2
        self.latency = self.border                       # energy.ml:432
        self.rate = (1, self.hop)                        # energy.ml:445
        self.reset()

    def reset(self):
        self._started = False
        self._drained = False
        self._pending = None
        self._tail = None
        self._skip = 0

    def _process(self, extra, borrowed):
        """energy.ml:232-259: ``extra`` joins the pending stream; the frames that became complete are emitted."""
        parts = ([] if self._pending is None else [self._pending]) + extra
        fresh = len(parts) > 1 or not borrowed
        samples = parts[0] if len(parts) == 1 else _join(parts)
        total = _length(samples)
        fl, hop = self.frame_length, self.hop
        count = 0 if total < fl else 1 + (total - fl) // hop
        if count == 0:
            self._pending = samples if fresh else _copy(samples)
            return None
        out = self._segment(samples, count)
        next_start = count * hop
        if next_start >= total:
            self._skip += next_start - total
            self._pending = None
        else:
            self._pending = _copy(samples[..., next_start:])
        return out

    def _segment(self, samples, count):
        """frames [0, count) of a segment of the padded stream"""
        return segment_frames(self.op, samples, count, self.frame_length, self.hop, self.threshold)

    def step(self, chunk):
        if self._drained:
            raise _lib.InvalidArgument("step: cannot feed a drained kernel (flush consumed the tail; reset before reusing)")
        shape = tuple(chunk.shape)
        if len(shape) < 1:
            raise _lib.InvalidArgument("step: cannot analyse a rank-zero tensor (the time axis must exist)")
        if 0 in shape[:-1]:
            raise _lib.InvalidArgument("step: cannot analyse a chunk with a zero-size leading axis (channels must be at least 1)")
        m = int(shape[-1])
        if m == 0:
            return None
        b = Batch(chunk, self.name)
        _refuse_device_float64(self.name, b)
        chunk = b.data if b.device or not b.torch else b.wrap(b.data)   # float32 / float64, contiguous, the caller's container
        self._tail = _copy(chunk[..., m - 1:])
        if not self._started:
            self._started = True
            if self.border == 0:
                return self._process([chunk], True)
            left = _zeros_like_lead(chunk, self.border) if self.op == RMS else _repeat(chunk[..., :1], self.border)
            return self._process([left, chunk], True)
        if self._skip >= m:
            self._skip -= m
            return None
        dropped, self._skip = self._skip, 0
        return self._process([chunk[..., dropped:] if dropped else chunk], True)

    __call__ = step

    def flush(self):
        if self._drained:
            return []
        self._drained = True
        out = None
        if self._started and self.border > 0:
            right = _zeros_like_lead(self._tail, self.border) if self.op == RMS else _repeat(self._tail, self.border)
            if self._skip >= self.border:
                self._skip -= self.border
            else:
                dropped, self._skip = self._skip, 0
                out = self._process([right[..., dropped:] if dropped else right], False)
        self._pending = None
        return [] if out is None else [out]


def rms_stage(frame_length: int = 2048, hop: int = 512):
    """``Soundml.rms_stage ?frame_length ?hop ()`` (energy.ml:514-517)."""
    return EnergyStage(RMS, frame_length, hop)


def zero_crossing_rate_stage(frame_length: int = 2048, hop: int = 512, threshold: float = 1e-10):
    """``Soundml.zero_crossing_rate_stage ?frame_length ?hop ?threshold ()`` (energy.ml:519-525)."""
    return EnergyStage(ZCR, frame_length, hop, threshold)
