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

from . import _lib
from ._lib import check, lib
from ._tensor import OUT, STREAM, Batch, FramedStage, prod, refuse_device_float64

RMS, ZCR = 0, 1
_NAMES = {RMS: "rms", ZCR: "zero_crossing_rate"}


def frames(n: int, frame_length: int = 2048, hop: int = 512) -> int:
    """The frame count of a length-``n`` signal (energy.ml:114-118): none for an empty one."""
    n, frame_length, hop = int(n), int(frame_length), int(hop)
    if n == 0:
        return 0
    padded = n + 2 * (frame_length // 2)
    return 0 if padded < frame_length else 1 + (padded - frame_length) // hop


def _centred(op, x, frame_length, hop, threshold):
    name = _NAMES[op]
    fl, hop, threshold = int(frame_length), int(hop), float(threshold)
    if op == RMS:
        host, device, params = (lib.smx_rms_f32, lib.smx_rms_f64), lib.smx_rms_device_f32, (fl, hop)
    else:
        host, device, params = ((lib.smx_zero_crossing_rate_f32, lib.smx_zero_crossing_rate_f64),
                                lib.smx_zero_crossing_rate_device_f32, (fl, hop, threshold))
    check(host[0](None, 0, 0, *params, None))            # the parameters come before the tensor is looked at: let the ABI word them
    b = Batch(x, name)
    refuse_device_float64(name, b)
    n = int(b.shape[-1])
    lead_shape = b.shape[:-1]
    lead = prod(lead_shape)
    count = frames(n, fl, hop)
    return b.run(host, (b.ptr(), lead, n, *params, OUT), device, (b.ptr(), lead, n, n, *params, OUT, STREAM), lead_shape + (1, count),
                 skip=lead == 0 or count == 0)           # energy.ml:354-366 `frameless`: zeros, no launch


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
    refuse_device_float64(op, b, "spectrograms are")
    return b.run((lib.smx_rms_of_spectrogram_f32, lib.smx_rms_of_spectrogram_f64), (b.ptr(), lead, bins, count, fl, OUT),
                 lib.smx_rms_of_spectrogram_device_f32, (b.ptr(), lead, bins, count, fl, OUT, STREAM), lead_shape + (1, count),
                 skip=lead == 0 or count == 0)


def segment_frames(op: int, samples, count: int, frame_length: int, hop: int, threshold: float = 0.0):
    """Frames [0, count) of a segment of the padded stream, no border (energy.ml:157-183 `analyse`): the stages' body.
    [...; n] -> [...; 1; count]; (count - 1) * hop + frame_length <= n."""
    name = _NAMES[op] + "_stage"
    b = Batch(samples, name)
    refuse_device_float64(name, b)
    n, count = int(b.shape[-1]), int(count)
    lead_shape = b.shape[:-1]
    lead = prod(lead_shape)
    args = (int(op), float(threshold), int(frame_length), int(hop))
    skip = lead == 0 or count == 0
    if skip:
        check(lib.smx_energy_frames_f32(*args, None, lead, n, count, None))
    return b.run((lib.smx_energy_frames_f32, lib.smx_energy_frames_f64), (*args, b.ptr(), lead, n, count, OUT),
                 lib.smx_energy_frames_device_f32, (*args, b.ptr(), lead, n, n, count, OUT, STREAM), lead_shape + (1, count), skip=skip)


class EnergyStage(FramedStage):
    """``rms_stage`` / ``zero_crossing_rate_stage`` (energy.ml:194-347): the framed-stream carry over ``segment_frames``, zero
    borders for rms and edge borders for the zero-crossing rate."""

    def __init__(self, op: int, frame_length: int = 2048, hop: int = 512, threshold: float = 0.0):
        self.op, self.threshold = int(op), float(threshold)
        # energy.ml:514-525: frame_length, hop, then the threshold, worded by the ABI
        check(lib.smx_energy_frames_f32(self.op, self.threshold, int(frame_length), int(hop), None, 0, 0, 0, None))
        super().__init__(_NAMES[self.op] + "_stage", frame_length, hop, "zeros" if self.op == RMS else "edge")

    def _segment(self, samples, count):
        return segment_frames(self.op, samples, count, self.frame_length, self.hop, self.threshold)


def rms_stage(frame_length: int = 2048, hop: int = 512):
    """``Soundml.rms_stage ?frame_length ?hop ()`` (energy.ml:514-517)."""
    return EnergyStage(RMS, frame_length, hop)


def zero_crossing_rate_stage(frame_length: int = 2048, hop: int = 512, threshold: float = 1e-10):
    """``Soundml.zero_crossing_rate_stage ?frame_length ?hop ?threshold ()`` (energy.ml:519-525)."""
    return EnergyStage(ZCR, frame_length, hop, threshold)
