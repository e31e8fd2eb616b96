"""Pitch on MI355X: YIN fundamental-frequency tracking (de Cheveigne & Kawahara 2002), exported flat as ``yin`` /
``yin_difference`` / ``yin_stage``.  The reference has no such module; the parameters carry the usual names.

    f0 = yin(x, fmin=65, fmax=2093, sample_rate=22050)                     # [...; n] -> [...; 1; frames]
    f0, ap = yin(x, 65, 2093, return_aperiodicity=True)                    # the voicing measure d'(tau) next to it
    d = yin_difference(x, 65, 2093)                                        # [...; n] -> [...; pmax + 1; frames]
    stage = yin_stage(65, 2093)                                            # audio chunks [...; m] -> [...; 1; k] | None; flush() -> list

The frame grid is that of ``rms``: the signal is centred by ``frame_length // 2`` virtual zeros on each side and frames advance
by ``hop`` (``frame_length // 4`` when ``None``).  Float64 inside, one rounding to the dtype of the input.  The correlation and the
energies of a frame have one summation order, a function of its own samples, so a leading slice of a batch, a
range of frames and any chunking of the stage give the flat call's values bit for bit (include/soundml_amd.h words the
definition).
"""
from __future__ import annotations

import math

from ._lib import check, lib
from ._tensor import Batch, out_ptr, prod
from .energy import EnergyStage, RMS, _refuse_device_float64, _zeros, frames       # noqa: F401  (frames: the grid is rms')


def _hop(frame_length, hop):
    return int(frame_length) // 4 if hop is None else int(hop)


def lag_range(sample_rate: int, fmin: float, fmax: float, frame_length: int = 2048):
    """(pmin, pmax): the lags searched, ``floor(sample_rate / fmax)`` to ``ceil(sample_rate / fmin)``, the latter capped at
    ``frame_length - frame_length // 2 - 1``; the ABI checks the parameters and words what is wrong with them."""
    sr, fl, fmin, fmax = int(sample_rate), int(frame_length), float(fmin), float(fmax)
    check(lib.smx_yin_difference_f32(None, 0, 0, sr, fmin, fmax, fl, 1, None))
    longest, cap = sr / fmin, fl - fl // 2 - 1
    return int(math.floor(sr / fmax)), cap if longest >= cap else int(math.ceil(longest))


def _run(name, x, params, count_of, host, resident, want_ap):
    """one frame call: the parameters are checked before the tensor is looked at"""
    b = Batch(x, name)
    _refuse_device_float64(name, b)
    n = int(b.shape[-1])
    lead_shape = b.shape[:-1]
    lead = prod(lead_shape)
    count = count_of(n)
    shape = lead_shape + (1, count)
    if lead == 0 or count == 0:
        f0 = _zeros(b, shape)
        return (f0, _zeros(b, shape)) if want_ap else f0
    f0 = b.empty(shape)
    ap = b.empty(shape) if want_ap else None
    if b.device:
        with b.device_guard():
            check(resident(b.ptr(), lead, n, n, *params, out_ptr(f0), out_ptr(ap) if want_ap else None, b.stream()))
        return (f0, ap) if want_ap else f0
    check(host[b.bytes](b.ptr(), lead, n, *params, out_ptr(f0), out_ptr(ap) if want_ap else None))
    return (b.wrap(f0), b.wrap(ap)) if want_ap else b.wrap(f0)


def yin(x, fmin: float, fmax: float, sample_rate: int = 22050, frame_length: int = 2048, hop=None, trough_threshold: float = 0.1,
        return_aperiodicity: bool = False):
    """Frame-wise fundamental frequency [...; n] -> [...; 1; frames]: per frame the first lag in
    ``[sample_rate / fmax, sample_rate / fmin]`` at which the cumulative-mean-normalised difference d' has a trough below
    ``trough_threshold`` (the lag of its minimum if there is none), refined by a parabola through its neighbours.  With
    ``return_aperiodicity`` also d' at that lag: near 0 for a periodic frame, 1 for silence.  A frame that holds a non-finite
    sample gives NaN in both."""
    fl, hop = int(frame_length), _hop(frame_length, hop)
    params = (int(sample_rate), float(fmin), float(fmax), fl, hop, float(trough_threshold))
    check(lib.smx_yin_f32(None, 0, 0, *params, None, None))
    return _run("yin", x, params, lambda n: frames(n, fl, hop), {4: lib.smx_yin_f32, 8: lib.smx_yin_f64}, lib.smx_yin_resident_f32,
                bool(return_aperiodicity))


def yin_difference(x, fmin: float, fmax: float, sample_rate: int = 22050, frame_length: int = 2048, hop=None):
    """The cumulative-mean-normalised difference d'(tau), tau = 0 .. pmax, of every frame: [...; n] -> [...; pmax + 1; frames]
    (``lag_range`` gives pmax)."""
    name = "yin_difference"
    fl, hop = int(frame_length), _hop(frame_length, hop)
    params = (int(sample_rate), float(fmin), float(fmax), fl, hop)
    check(lib.smx_yin_difference_f32(None, 0, 0, *params, None))
    lags = lag_range(sample_rate, fmin, fmax, fl)[1] + 1
    b = Batch(x, name)
    _refuse_device_float64(name, b)
    n = int(b.shape[-1])
    lead_shape = b.shape[:-1]
    lead = prod(lead_shape)
    count = frames(n, fl, hop)
    if lead == 0 or count == 0:
        return _zeros(b, lead_shape + (lags, count))
    out = b.empty(lead_shape + (lags, count))
    if b.device:
        with b.device_guard():
            check(lib.smx_yin_difference_resident_f32(b.ptr(), lead, n, n, *params, out_ptr(out), b.stream()))
        return out
    fn = lib.smx_yin_difference_f32 if b.bytes == 4 else lib.smx_yin_difference_f64
    check(fn(b.ptr(), lead, n, *params, out_ptr(out)))
    return b.wrap(out)


def segment_frames(samples, count: int, fmin: float, fmax: float, sample_rate: int = 22050, frame_length: int = 2048, hop=None,
                   trough_threshold: float = 0.1, return_aperiodicity: bool = False):
    """Frames [0, count) of a segment of the padded stream, no border: the stage's body.  [...; n] -> [...; 1; count];
    (count - 1) * hop + frame_length <= n."""
    fl, hop, count = int(frame_length), _hop(frame_length, hop), int(count)
    params = (count, int(sample_rate), float(fmin), float(fmax), fl, hop, float(trough_threshold))
    check(lib.smx_yin_frames_f32(None, 0, 0, 0, *params[1:], None, None))
    return _run("yin_stage", samples, params, lambda n: count, {4: lib.smx_yin_frames_f32, 8: lib.smx_yin_frames_f64},
                lib.smx_yin_frames_resident_f32, bool(return_aperiodicity))


class YinStage(EnergyStage):
    """The streaming form of ``yin``: the carry of the energy stages (the pending suffix of the padded stream, the skip when the
    hop outruns the data, zero borders as rms') over this module's segment call.  Only shapes decide the control flow: device
    chunks cause no synchronisation.  A step returns [...; 1; k], a pair with ``return_aperiodicity``, or None."""

    def __init__(self, fmin: float, fmax: float, sample_rate: int = 22050, frame_length: int = 2048, hop=None,
                 trough_threshold: float = 0.1, return_aperiodicity: bool = False):
        self.op = RMS                                    # the borders are zeros
        self.name = "yin_stage"
        self.frame_length, self.hop, self.threshold = int(frame_length), _hop(frame_length, hop), float(trough_threshold)
        self.fmin, self.fmax, self.sample_rate = float(fmin), float(fmax), int(sample_rate)
        self.return_aperiodicity = bool(return_aperiodicity)
        check(lib.smx_yin_frames_f32(None, 0, 0, 0, self.sample_rate, self.fmin, self.fmax, self.frame_length, self.hop, self.threshold,
                                     None, None))
        self.border = self.frame_length // 2
        self.latency = self.border
        self.rate = (1, self.hop)
        self.reset()

    def _segment(self, samples, count):
        return segment_frames(samples, count, self.fmin, self.fmax, self.sample_rate, self.frame_length, self.hop, self.threshold,
                              self.return_aperiodicity)


def yin_stage(fmin: float, fmax: float, sample_rate: int = 22050, frame_length: int = 2048, hop=None, trough_threshold: float = 0.1,
              return_aperiodicity: bool = False):
    """``yin`` over a stream of chunks: ``step`` / ``flush`` / ``reset``, latency ``frame_length // 2``, rate ``(1, hop)``."""
    return YinStage(fmin, fmax, sample_rate, frame_length, hop, trough_threshold, return_aperiodicity)
