"""Per-channel energy normalisation on MI355X (PCEN: Wang et al. 2017, Lostanlen et al. 2019; ``librosa.pcen`` with ``max_size=1``;
the reference has no such module): the usual replacement for log-mel in keyword spotting, bioacoustics and far-field speech.

    c = Pcen.Config.create(sr=22050, hop=512, gain=0.98, bias=2.0, power=0.5, time_constant=0.4, eps=1e-6, b=None, scale=1.0)
    P = Pcen.apply(c, S)                                  # [...; bands; frames] -> the same shape; S non-negative and finite
    P, zf = Pcen.apply(c, S, zi=zi, return_state=True)    # zi, zf [...; bands] float64: the smoother before / at the last frame
    M = Pcen.smooth(c, S)                                 # the smoother alone, rounded once to the dtype of S
    P = pcen(stft_config, mel_config, x, c)               # [...; n] -> [...; n_mels; frames]: apply of mel_spectrogram(power=1.0)
    k = Pcen.Kernel.prepare(c, *lead_shape)               # k.step(chunk [...; bands; m]) -> the same shape | None; k.flush() -> []

Float64 inside, one rounding to the dtype of the input.  ``u = scale * S`` (librosa's convention for float audio is ``scale=2**31``),
``M[t] = (1 - s) M[t-1] + s u[t]`` from ``M[-1] = zi`` or ``u[0]``, then librosa's stable form of ``(u / (eps + M)**gain + bias)**power
- bias**power`` (DESIGN.md 4.8m states every operation).  Time is not cut into blocks, so both kernels, a leading slice of a batch, a
call continued from another call's ``zf`` and every chunking of a ``Kernel`` give the same bits.  ``max_size > 1`` and per-band
parameters are out of scope.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import check, lib
from ._tensor import OUT, STREAM, Batch, is_device, is_torch, out_ptr, prod, refuse_device_float64, torch

TILE_MIN_FRAMES = int(lib.smx_pcen_tile_min_frames())      # calls of at least this many frames take the tile kernel


class Config:
    def __init__(self, handle, **params):
        self._h = handle
        self.__dict__.update(params)

    @staticmethod
    def create(sr=22050, hop=512, gain=0.98, bias=2.0, power=0.5, time_constant=0.4, eps=1e-6, b=None, scale=1.0) -> "Config":
        params = dict(sr=int(sr), hop=int(hop), gain=float(gain), bias=float(bias), power=float(power), time_constant=float(time_constant),
                      eps=float(eps), b=None if b is None else float(b), scale=float(scale))
        handle = C.c_void_p()
        check(lib.smx_pcen_create(params["sr"], params["hop"], params["gain"], params["bias"], params["power"], params["time_constant"], params["eps"],
                                  0 if b is None else 1, 0.0 if b is None else params["b"], params["scale"], C.byref(handle)))
        return Config(handle, **params)

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h and lib is not None:
            try:
                lib.smx_pcen_destroy(h)
            except Exception:
                pass

    coefficient = property(lambda self: float(lib.smx_pcen_coefficient(self._h)))


def _spectrogram(op, S):
    if len(tuple(S.shape)) < 2:
        raise _lib.InvalidArgument("%s: cannot normalise a tensor of rank %d (the band and frame axes must exist: [...; bands; frames])"
                                   % (op, len(tuple(S.shape))))
    b = Batch(S, op)
    refuse_device_float64(op, b, "spectrograms are")
    return b


def _state(op, b, zi):
    """zi on the side of the spectrogram: a float64 device tensor or numpy array [...; bands], or None"""
    if zi is None:
        return None
    want = tuple(b.shape[:-1])
    if tuple(zi.shape if hasattr(zi, "shape") else np.shape(zi)) != want:
        raise _lib.InvalidArgument("%s: cannot start from a state of shape %s (zi must be one value per row, %s)"
                                   % (op, tuple(np.shape(zi) if not hasattr(zi, "shape") else zi.shape), want))
    if b.device:
        if is_device(zi):
            return zi.to(device=b.data.device, dtype=torch.float64).contiguous()      # already resident: no wait
        z = zi.detach().numpy() if is_torch(zi) else np.asarray(zi)
        return torch.from_numpy(np.ascontiguousarray(z, dtype=np.float64)).to(b.data.device)
    z = zi.detach().cpu().numpy() if is_torch(zi) else np.asarray(zi)
    return np.ascontiguousarray(z, dtype=np.float64)


def _run(op, c, S, zi, return_state, host, device, takes_zf):
    b = _spectrogram(op, S)
    frames, row_shape = int(b.shape[-1]), tuple(b.shape[:-1])
    rows = prod(row_shape)
    z = _state(op, b, zi)
    if rows == 0 or frames == 0:                          # nothing to normalise: no launch, the state given is the state returned
        out = b.wrap(b.empty(b.shape))
        if not return_state:
            return out
        if b.device:
            return out, (torch.zeros(row_shape, dtype=torch.float64, device=b.data.device) if z is None else z.clone())
        return out, b.wrap(np.zeros(row_shape) if z is None else z.copy())
    zf = None                                             # the float64 states lie on the spectrogram's side
    if return_state:
        zf = torch.empty(row_shape, dtype=torch.float64, device=b.data.device) if b.device else np.zeros(row_shape)
    ptr = lambda t: None if t is None else out_ptr(t)
    tail = (ptr(zf),) if takes_zf else ()
    out = b.run(host, (c._h, b.ptr(), rows, frames, ptr(z), OUT) + tail,
                device, (c._h, STREAM, b.ptr(), rows, frames, frames, ptr(z), OUT) + tail, b.shape, overwritten=True)
    if b.device and z is not None:
        z.record_stream(torch.cuda.current_stream(b.data.device))
    return (out, b.wrap(zf)) if return_state else out


def apply(c: Config, S, zi=None, return_state: bool = False):
    """PCEN along the last axis: [...; bands; frames] -> the same shape (and ``M`` at the last frame, [...; bands] float64)."""
    return _run("apply", c, S, zi, return_state, (lib.smx_pcen_apply_f32, lib.smx_pcen_apply_f64), lib.smx_pcen_apply_card_f32, True)


def smooth(c: Config, S, zi=None):
    """The smoother alone: ``M`` [...; bands; frames], rounded once to the dtype of ``S``."""
    return _run("smooth", c, S, zi, False, (lib.smx_pcen_smooth_f32, lib.smx_pcen_smooth_f64), lib.smx_pcen_smooth_card_f32, False)


def pcen(stft_config, mel_config, x, c: Config):
    """``Pcen.apply(c, mel_spectrogram(stft_config, mel_config, x, power=1.0))`` bit for bit, the mel spectrogram never leaving the
    device: [...; n] -> [...; n_mels; frames]."""
    from . import stft as Stft
    b = Batch(x, "pcen")
    refuse_device_float64("pcen", b)
    n, lead_shape = int(b.shape[-1]), b.shape[:-1]
    lead = prod(lead_shape)
    count = Stft.frames(stft_config, n)
    cfgs = (stft_config._h, mel_config._h)
    return b.run((lib.smx_pcen_of_audio_f32, lib.smx_pcen_of_audio_f64), (c._h, *cfgs, b.ptr(), lead, n, OUT),
                 lib.smx_pcen_of_audio_card_f32, (c._h, STREAM, *cfgs, b.ptr(), lead, n, n, OUT), lead_shape + (mel_config.n_mels, count))


class Kernel:
    """The streaming form: one double per row stays on the device (``M`` at the last frame fed); whether the stream has started is a
    host boolean.  ``step`` returns as many frames as it is given (latency zero); the first non-empty step starts the smoother from
    its own first column, and the concatenated steps equal ``apply`` of the whole spectrogram bit for bit under every chunking.
    Only shapes decide the control flow: device chunks cause no synchronisation.  The state is input and output of every step: a
    kernel belongs to the device of its first step and to one stream at a time."""
    latency = 0
    rate = (1, 1)

    def __init__(self, handle, config, lead_shape):
        self._h, self.config, self.lead_shape = handle, config, tuple(lead_shape)

    @staticmethod
    def prepare(c: Config, *lead_shape) -> "Kernel":
        if len(lead_shape) == 1 and isinstance(lead_shape[0], (tuple, list)):
            lead_shape = tuple(lead_shape[0])
        lead_shape = tuple(int(d) for d in lead_shape)
        if len(lead_shape) < 1:
            raise _lib.InvalidArgument("prepare: cannot keep the state of a stream without a band axis (lead_shape must end in the number of bands)")
        handle = C.c_void_p()
        check(lib.smx_pcen_kernel_prepare(c._h, prod(lead_shape), C.byref(handle)))
        return Kernel(handle, c, lead_shape)

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h and lib is not None:
            try:
                lib.smx_pcen_kernel_destroy(h)
            except Exception:
                pass

    def reset(self):
        check(lib.smx_pcen_kernel_reset(self._h))

    def step(self, chunk):
        shape = tuple(chunk.shape)
        if len(shape) < 2:
            raise _lib.InvalidArgument("step: cannot normalise a tensor of rank %d (the band and frame axes must exist: [...; bands; frames])" % len(shape))
        m = int(shape[-1])
        if m == 0:
            check(lib.smx_pcen_kernel_step_f32(self._h, None, 0, None))     # a drained kernel refuses an empty chunk too
            return None
        if shape[:-1] != self.lead_shape:
            raise _lib.InvalidArgument("step: cannot normalise a chunk of leading shape %s with a kernel prepared for %s"
                                       % (shape[:-1], self.lead_shape))
        b = Batch(chunk, "step")
        refuse_device_float64("step", b, "spectrograms are")
        return b.run((lib.smx_pcen_kernel_step_f32, lib.smx_pcen_kernel_step_f64), (self._h, b.ptr(), m, OUT),
                     lib.smx_pcen_kernel_step_card_f32, (self._h, STREAM, b.ptr(), m, m, OUT), b.shape, overwritten=True)

    __call__ = step

    def flush(self):
        check(lib.smx_pcen_kernel_flush(self._h))
        return []
