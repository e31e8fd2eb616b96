"""Programme loudness and true peak on MI355X (ITU-R BS.1770-4; the meter's windows and compliance signals: EBU Tech 3341; the
reference has no such module).

    sos = Loudness.k_weighting(rate)                    # [2; 6] float64: the shelf and the RLB high-pass at any rate >= 8000
    z = Loudness.block_energy(x, rate)                  # [...; channels; n] -> [...; channels; nb] float64, 400 ms blocks, 100 ms hop
    m = Loudness.momentary(x, rate, weights=None)       # -> [...; nb] LUFS;  Loudness.short_term: 3 s windows, [...; max(0, nb - 26)]
    i = Loudness.integrated(x, rate, weights=None)      # -> [...] LUFS, gated (-70 LUFS absolute, -10 LU relative); -inf when nothing passes
    p = Loudness.true_peak(x)                           # -> [...; channels], linear; Convert.amplitude_to_db gives dBTP
    y = Loudness.normalize(x, rate, target=-23.0, peak_ceiling=None)      # one gain per clip, on the device
    k = Loudness.Meter.prepare(rate, 2)                 # k.step(chunk) -> [...; blocks completed] | None; k.integrated(); k.short_term()

The channel axis is always there ([1; n] for mono).  ``weights`` are the channel gains G_c (``Loudness.SURROUND_5_0`` for L R C Ls Rs;
a weight of 0 drops a channel).  The K-weighted signal is Iir's stated order in float64 and is never rounded or
stored; every sum behind a result has one stated order, so both kernels, a leading slice of a batch and every
chunking of a ``Meter`` give the same bits.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import check, lib
from ._tensor import OUT, STREAM, Batch, out_ptr, prod, refuse_device_float64, torch

MIN_RATE = int(lib.smx_loudness_min_rate())
MAX_CHANNELS = int(lib.smx_loudness_max_channels())
ABSOLUTE_GATE = float(lib.smx_loudness_absolute_gate())      # E_abs = 10^((-70 + 0.691) / 10)
SURROUND_5_0 = (1.0, 1.0, 1.0, 1.41, 1.41)                   # L R C Ls Rs (BS.1770-4 table 3)

_refuse_device_float64 = refuse_device_float64


def _rate(op: str, rate) -> int:
    rate = int(rate)
    if rate < MIN_RATE:
        raise _lib.InvalidArgument("%s: cannot meter audio at %d Hz (rate must be at least %d)" % (op, rate, MIN_RATE))
    return rate


def step(rate) -> int:
    """samples between gating blocks: 100 ms, (rate + 5) // 10"""
    return int(lib.smx_loudness_step(int(rate)))


def blocks(rate, n) -> int:
    """whole 400 ms gating blocks in n samples"""
    return int(lib.smx_loudness_blocks(int(rate), int(n)))


def k_weighting(rate) -> np.ndarray:
    """BS.1770-4's two sections at ``rate``, [2; 6] float64 rows b0 b1 b2 1 a1 a2 (``Iir.Config.create`` takes them)."""
    sos = np.empty((2, 6), np.float64)
    check(lib.smx_loudness_k_weighting(int(rate), C.c_void_p(sos.ctypes.data)))
    return sos


def true_peak_taps() -> np.ndarray:
    """h[k] = sinc((k - 24) / 4) kaiser(49, 8.0)[k], scaled to sum 4: the 4x oversampler of ``true_peak``, [49] float64."""
    h = np.empty(49, np.float64)
    check(lib.smx_loudness_true_peak_taps(C.c_void_p(h.ctypes.data)))
    return h


class _Audio:
    """[...; channels; n] behind a Batch: the extents, and the weights as the ABI takes them"""

    def __init__(self, x, op, rate=None, weights=None):
        self.b = b = Batch(x, op)
        if len(b.shape) < 2:
            raise _lib.InvalidArgument("%s: cannot meter a tensor of shape %s (audio is [...; channels; n]: the channel axis must exist, [1; n] for mono)"
                                       % (op, tuple(b.shape)))
        _refuse_device_float64(op, b)
        self.rate = None if rate is None else _rate(op, rate)
        self.lead_shape, self.channels, self.n = tuple(b.shape[:-2]), int(b.shape[-2]), int(b.shape[-1])
        self.clips = prod(self.lead_shape)
        self.weights, self.wp = _weights(op, weights, self.channels)
        self.nb = 0 if rate is None else blocks(self.rate, self.n)


def _weights(op, weights, channels):
    if not 1 <= channels <= MAX_CHANNELS:
        raise _lib.InvalidArgument("%s: cannot meter %d channels (channels must lie in [1, %d])" % (op, channels, MAX_CHANNELS))
    if weights is None:
        return None, None
    w = np.ascontiguousarray(np.asarray(weights, dtype=np.float64).reshape(-1))
    if w.shape[0] != channels:
        raise _lib.InvalidArgument("%s: cannot weight %d channels with %d weights (weights must have one entry per channel)" % (op, channels, w.shape[0]))
    return w, C.c_void_p(w.ctypes.data)


def _float64_out(b, shape):
    if b.device:
        return torch.empty(shape, dtype=torch.float64, device=b.data.device)
    return np.zeros(shape, np.float64)


def block_energy(x, rate):
    """z[c, j]: the mean square of channel c's K-weighted signal over gating block j, [...; channels; nb] float64."""
    a = _Audio(x, "block_energy", rate)
    b = a.b
    z = _float64_out(b, a.lead_shape + (a.channels, a.nb))
    if a.clips and a.nb:
        b.run((lib.smx_loudness_block_energy_f32, lib.smx_loudness_block_energy_f64), (b.ptr(), a.clips, a.channels, a.n, a.rate, out_ptr(z)),
              lib.smx_loudness_block_energy_card_f32, (b.ptr(), STREAM, a.clips, a.channels, a.n, a.n, a.rate, out_ptr(z)), [])
    return b.wrap(z)


def _windows(op, x, rate, weights, short_term):
    a = _Audio(x, op, rate, weights)
    b = a.b
    count = max(0, a.nb - 26) if short_term else a.nb
    return b.run((lib.smx_loudness_momentary_f32, lib.smx_loudness_momentary_f64), (b.ptr(), a.clips, a.channels, a.n, a.rate, a.wp, short_term, OUT),
                 lib.smx_loudness_momentary_card_f32, (b.ptr(), STREAM, a.clips, a.channels, a.n, a.n, a.rate, a.wp, short_term, OUT),
                 a.lead_shape + (count,), skip=a.clips == 0 or count == 0, overwritten=True)


def momentary(x, rate, weights=None):
    """-0.691 + 10 log10(sum_c G_c z[c, j]) per 400 ms block: [...; channels; n] -> [...; nb] LUFS in the dtype of the input."""
    return _windows("momentary", x, rate, weights, 0)


def short_term(x, rate, weights=None):
    """The same over 3 s windows (30 steps) at the 100 ms hop: -> [...; max(0, nb - 26)]."""
    return _windows("short_term", x, rate, weights, 1)


def integrated(x, rate, weights=None):
    """Gated programme loudness (BS.1770-4): [...; channels; n] -> [...] LUFS; -inf when no block passes both gates."""
    a = _Audio(x, "integrated", rate, weights)
    b = a.b
    return b.run((lib.smx_loudness_integrated_f32, lib.smx_loudness_integrated_f64), (b.ptr(), a.clips, a.channels, a.n, a.rate, a.wp, OUT, None),
                 lib.smx_loudness_integrated_card_f32, (b.ptr(), STREAM, a.clips, a.channels, a.n, a.n, a.rate, a.wp, OUT, None),
                 a.lead_shape, skip=a.clips == 0, overwritten=True)


def gate_mask(x, rate, weights=None):
    """The gates' verdict per block, [...; nb] uint8: bit 0 through the absolute gate, bit 1 through both (a debug face)."""
    a = _Audio(x, "integrated", rate, weights)
    b = a.b
    shape = a.lead_shape + (a.nb,)
    mask = torch.zeros(shape, dtype=torch.uint8, device=b.data.device) if b.device else np.zeros(shape, np.uint8)
    if a.clips and a.nb:
        b.run((lib.smx_loudness_integrated_f32, lib.smx_loudness_integrated_f64), (b.ptr(), a.clips, a.channels, a.n, a.rate, a.wp, OUT, out_ptr(mask)),
              lib.smx_loudness_integrated_card_f32, (b.ptr(), STREAM, a.clips, a.channels, a.n, a.n, a.rate, a.wp, OUT, out_ptr(mask)), a.lead_shape)
    return b.wrap(mask)


def true_peak(x):
    """max |y| of the 4x oversampled signal per channel: [...; channels; n] -> [...; channels], a linear amplitude."""
    a = _Audio(x, "true_peak")
    b = a.b
    rows = a.clips * a.channels
    return b.run((lib.smx_loudness_true_peak_f32, lib.smx_loudness_true_peak_f64), (b.ptr(), rows, a.n, OUT),
                 lib.smx_loudness_true_peak_card_f32, (b.ptr(), STREAM, rows, a.n, a.n, OUT), a.lead_shape + (a.channels,), skip=rows == 0,
                 overwritten=True)


def normalize(x, rate, target: float = -23.0, peak_ceiling=None, weights=None):
    """x times one gain per clip, 10^((target - integrated) / 20), lowered until gain * max_c true_peak <= peak_ceiling (a linear
    amplitude) when one is given; a clip at -inf keeps gain 1.  The gain is computed and applied on the device in float64."""
    a = _Audio(x, "normalize", rate, weights)
    b = a.b
    has, ceiling = (0, 0.0) if peak_ceiling is None else (1, float(peak_ceiling))
    if has and not (ceiling > 0.0 and np.isfinite(ceiling)):
        raise _lib.InvalidArgument("normalize: cannot hold peaks under %g (peak_ceiling is a linear amplitude: positive and finite)" % ceiling)
    return b.run((lib.smx_loudness_normalize_f32, lib.smx_loudness_normalize_f64),
                 (b.ptr(), a.clips, a.channels, a.n, a.rate, float(target), has, ceiling, a.wp, OUT),
                 lib.smx_loudness_normalize_card_f32, (b.ptr(), STREAM, a.clips, a.channels, a.n, a.n, a.rate, float(target), has, ceiling, a.wp, OUT),
                 b.shape, skip=a.clips == 0 or a.n == 0, empty="uninitialised", overwritten=True)


class Meter:
    """The streaming form.  Per channel Iir's record (4.8k), the partial energy of the open piece and the step energies so far stay
    on the device; the position is a host integer, and the host doubles the step buffer by shape alone.  ``step`` returns the
    momentary loudness of the blocks that completed, ``integrated()`` and ``short_term()`` read the step energies kept so far; the
    concatenated steps equal ``momentary`` of the whole signal and ``integrated()`` after the last step equals ``integrated`` of
    it, bit for bit under every chunking.  Only shapes decide the control flow: device chunks cause no synchronisation."""

    def __init__(self, handle, rate, lead_shape, channels):
        self._h, self.rate, self.lead_shape, self.channels = handle, rate, tuple(lead_shape), channels
        self._device, self._dtype, self._torch = None, np.dtype(np.float32), False

    @staticmethod
    def prepare(rate, *shape, weights=None) -> "Meter":
        """``shape`` is the chunks' shape without the time axis, channels last: ``prepare(48000, 2)`` meters [2; m] chunks."""
        if len(shape) == 1 and isinstance(shape[0], (tuple, list)):
            shape = tuple(shape[0])
        shape = tuple(int(d) for d in shape)
        rate = _rate("prepare", rate)
        if len(shape) < 1:
            raise _lib.InvalidArgument("prepare: cannot meter chunks of shape () (the channel axis must exist, 1 for mono)")
        _, wp = w = _weights("prepare", weights, shape[-1])
        handle = C.c_void_p()
        check(lib.smx_loudness_meter_prepare(rate, prod(shape[:-1]), shape[-1], wp, C.byref(handle)))
        del w
        return Meter(handle, rate, shape[:-1], shape[-1])

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h and lib is not None:
            try:
                lib.smx_loudness_meter_destroy(h)
            except Exception:
                pass

    position = property(lambda self: int(lib.smx_loudness_meter_position(self._h)))
    blocks = property(lambda self: max(0, self.position // step(self.rate) - 3))

    def reset(self):
        check(lib.smx_loudness_meter_reset(self._h))

    def step(self, chunk):
        shape = tuple(chunk.shape)
        if len(shape) < 2:
            raise _lib.InvalidArgument("step: cannot meter a tensor of shape %s (chunks are [...; channels; m])" % (shape,))
        m = int(shape[-1])
        if shape[:-1] != self.lead_shape + (self.channels,):
            raise _lib.InvalidArgument("step: cannot meter a chunk of leading shape %s with a meter prepared for %s"
                                       % (shape[:-1], self.lead_shape + (self.channels,)))
        if m == 0:
            check(lib.smx_loudness_meter_step_f32(self._h, None, 0, None))     # a drained meter refuses an empty chunk too
            return None
        b = Batch(chunk, "step")
        _refuse_device_float64("step", b)
        self._device, self._dtype, self._torch = (b.data.device if b.device else None), np.dtype(np.float32 if b.bytes == 4 else np.float64), b.torch
        before = self.blocks
        k = max(0, (self.position + m) // step(self.rate) - 3) - before
        out = b.run((lib.smx_loudness_meter_step_f32, lib.smx_loudness_meter_step_f64), (self._h, b.ptr(), m, OUT),
                    lib.smx_loudness_meter_step_card_f32, (self._h, STREAM, b.ptr(), m, m, OUT), [self.lead_shape + (k,) if k else None],
                    overwritten=True)[0]
        return out

    __call__ = step

    def flush(self):
        check(lib.smx_loudness_meter_flush(self._h))
        return []

    def _read(self, what, shape):
        if self._device is not None:
            out = torch.zeros(shape, dtype=torch.float32, device=self._device)
            if out.numel():
                with torch.cuda.device(self._device.index):
                    check(lib.smx_loudness_meter_read_card_f32(self._h, C.c_void_p(torch.cuda.current_stream(self._device.index).cuda_stream), what,
                                                               out_ptr(out)))
            return out
        out = np.zeros(shape, self._dtype)
        if out.size:
            check((lib.smx_loudness_meter_read_f32 if self._dtype == np.float32 else lib.smx_loudness_meter_read_f64)(self._h, what, out_ptr(out)))
        return torch.from_numpy(out) if self._torch else out

    def integrated(self):
        """-> [...] LUFS of everything fed so far, in the kind and dtype of the last chunk (host float32 before the first)."""
        return self._read(0, self.lead_shape)

    def short_term(self):
        """-> [...; max(0, blocks - 26)]: the 3 s windows complete so far."""
        return self._read(1, self.lead_shape + (max(0, self.blocks - 26),))
