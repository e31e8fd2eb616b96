"""``Soundml.Cqt``: the offline constant-Q / variable-Q transform on MI355X (reference: soundml/lib/cqt.ml, cqt.mli:64-315).

    c = Cqt.Config.create(n_bins=84, sample_rate=22050)            # C1 upward, 12 bins per octave, hop 512, zero padding
    z = Cqt.transform(c, x)                                          # [...; n] float32 -> [...; n_bins; frames] complex64
    s = Cqt.power_spectrum(c, x, power=1.0)                          # |z|^power, float32
    f, l = Cqt.frequencies(np.float64, c), Cqt.filter_lengths(np.float64, c)
    y = soundml_amd.chroma_cqt(c, x)                                 # Chroma.of_cqt of the magnitudes, on the device throughout

The plan is the reference's, built once on the host in float64 (no device needed): the octave-by-octave ladder, the
early decimations, one bank of filters per octave.  Each octave runs at the rate its filters need: the signal is halved
between octaves by ``Resample.Config.create(2, 1, "high")`` while the octave's hop is even, and every frame of the octave's
centered rectangular analysis is projected against the bank in float64 (one kernel launch per octave, one rounding).  Host
arrays give host arrays; device tensors stay on the device.

    k = Cqt.Kernel.prepare(c, channels=2, max_block=4096)          # the streaming face (cqt.mli:317-413)
    cols = [k.step(chunk) for chunk in chunks] + [k.flush()]         # None, or [...; n_bins; columns]; together: transform, bit for bit

``Cqt.Kernel`` holds one state for all channels on the device: the streaming 2:1 decimators, each octave's recent samples and a
ring of finished columns.  A column leaves in the step that completes its last octave (``columns_ready``); ``flush`` drains the
decimators and applies the right boundary rule.  The concatenation of every step plus flush equals ``transform`` (with
``power``: ``power_spectrum``) of the concatenated signal bit for bit under every chunking -- stronger than the reference, whose
two paths sum in different orders and agree to 2e-6.

DEVIATION: float32 audio only -- float64 raises, as ``Resample.apply`` does (the reference decimates either).
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _lib
from ._lib import check, lib
from ._tensor import OUT, STREAM, Batch, out_ptr, prod

C1 = 32.70319566257483
_GAMMA = {"constant_q": 0, "erb": 1}


def _g(v) -> str:
    v = float(v)
    if math.isnan(v):
        return "nan"
    if math.isinf(v):
        return "inf" if v > 0 else "-inf"
    return "%g" % v


class Config:
    """``Cqt.Config.t`` (cqt.ml:287-424).  ``gamma``: "constant_q" | "erb" | a non-negative float (`` `Fixed g``);
    ``window``: a family name or ``(name, shape)`` for "kaiser" / "gaussian" / "tukey"; ``pad``: "constant" (with
    ``pad_value``, the default 0) | "reflect" | "edge"."""

    def __init__(self, handle, params):
        self._h, self._params = handle, params

    @staticmethod
    def create(n_bins: int, sample_rate: int, fmin: float = C1, bins_per_octave: int = 12, gamma="constant_q", tuning: float = 0.0,
               filter_scale: float = 1.0, norm: float = 1.0, window="hann", scale: bool = True, hop: int = 512, pad: str = "constant",
               pad_value: float = 0.0) -> "Config":
        if isinstance(gamma, str):
            if gamma not in _GAMMA:
                raise _lib.InvalidArgument("create: cannot use gamma %r (one of 'constant_q', 'erb', or a non-negative number)" % (gamma,))
            gamma_kind, gamma_value = _GAMMA[gamma], 0.0
        else:
            gamma_kind, gamma_value = 2, float(gamma)
        if isinstance(pad, tuple):   # ("constant", v), as Stft.Config.create takes it
            pad, pad_value = pad[0], float(pad[1])
        name, shape = (window, 0.0) if isinstance(window, str) else (window[0], float(window[1]))
        if name not in _lib.WINDOW or name == "custom":
            raise _lib.InvalidArgument("create: unknown window family %r" % (name,))
        if pad not in _lib.PAD:
            raise _lib.InvalidArgument("create: unknown pad mode %r" % (pad,))
        handle = C.c_void_p()
        check(lib.smx_cqt_config_create(int(n_bins), int(sample_rate), float(fmin), int(bins_per_octave), gamma_kind, gamma_value,
                                        float(tuning), float(filter_scale), float(norm), _lib.WINDOW[name], shape, 1 if scale else 0,
                                        int(hop), _lib.PAD[pad], float(pad_value), C.byref(handle)))
        return Config(handle, dict(n_bins=int(n_bins), sample_rate=int(sample_rate), fmin=float(fmin), bins_per_octave=int(bins_per_octave),
                                   gamma=gamma if isinstance(gamma, str) else float(gamma), tuning=float(tuning),
                                   filter_scale=float(filter_scale), norm=float(norm),
                                   window=window if isinstance(window, str) else (name, shape), scale=bool(scale), hop=int(hop),
                                   pad=pad, pad_value=float(pad_value) if pad == "constant" else 0.0))

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h and lib is not None:
            try:
                lib.smx_cqt_config_destroy(h)
            except Exception:
                pass

    # cqt.mli:145-194
    n_bins = property(lambda self: lib.smx_cqt_config_n_bins(self._h))
    bins_per_octave = property(lambda self: lib.smx_cqt_config_bins_per_octave(self._h))
    sample_rate = property(lambda self: lib.smx_cqt_config_sample_rate(self._h))
    hop = property(lambda self: lib.smx_cqt_config_hop(self._h))
    fmin = property(lambda self: self._params["fmin"])
    gamma = property(lambda self: self._params["gamma"])
    tuning = property(lambda self: self._params["tuning"])
    filter_scale = property(lambda self: self._params["filter_scale"])
    norm = property(lambda self: self._params["norm"])
    window = property(lambda self: self._params["window"])
    scale = property(lambda self: self._params["scale"])
    pad = property(lambda self: self._params["pad"])
    pad_value = property(lambda self: self._params["pad_value"])
    n_octaves = property(lambda self: lib.smx_cqt_config_n_octaves(self._h))
    cutoff = property(lambda self: lib.smx_cqt_config_cutoff(self._h))
    latency = property(lambda self: lib.smx_cqt_config_latency(self._h),
                       doc="cqt.mli:196-231: max over octaves of D (L - 1) + K (D - 1) + 1 input samples")
    early = property(lambda self: lib.smx_cqt_config_early(self._h), doc="2:1 decimations before octave zero (cqt.ml:338-345)")

    @property
    def octaves(self):
        """The plan, highest octave first: ``(first, count, n_fft, hop, halvings)`` per octave (cqt.ml:78-85)."""
        out = []
        for i in range(self.n_octaves):
            v = [C.c_int64() for _ in range(5)]
            check(lib.smx_cqt_config_octave(self._h, i, *[C.byref(t) for t in v]))
            out.append(tuple(t.value for t in v))
        return out

    def taps(self, i: int) -> np.ndarray:
        """Octave ``i``'s filters as the device reads them: complex128 ``[count; n_fft]``, the time-domain form of the
        reference's half-spectrum kernel with the octave gain folded in."""
        _, count, n_fft, _, _ = self.octaves[i]
        out = np.empty((count, n_fft), dtype=np.complex128)
        check(lib.smx_cqt_config_taps(self._h, int(i), C.c_void_p(out.ctypes.data)))
        return out

    def divisors(self) -> np.ndarray:
        """The ``scale`` divisors, sqrt of the filter lengths at the rate octave zero runs at (ones when scale is off)."""
        out = np.empty(self.n_bins, dtype=np.float64)
        check(lib.smx_cqt_config_divisors(self._h, C.c_void_p(out.ctypes.data)))
        return out

    def __eq__(self, other):   # cqt.ml:505-528 equal
        return isinstance(other, Config) and self._params == other._params

    __hash__ = None

    def __repr__(self):        # cqt.ml:489-503 pp
        p = self._params
        gamma = p["gamma"] if isinstance(p["gamma"], str) else "fixed(%s)" % _g(p["gamma"])
        window = p["window"] if isinstance(p["window"], str) else "%s(%s)" % (p["window"][0], _g(p["window"][1]))
        pad = "constant(%s)" % _g(p["pad_value"]) if p["pad"] == "constant" else p["pad"]
        return ("cqt(n_bins=%d, bins_per_octave=%d, sample_rate=%d, fmin=%s, hop=%d, gamma=%s, tuning=%s, filter_scale=%s, norm=%s, "
                "window=%s, scale=%s, pad=%s)" % (p["n_bins"], p["bins_per_octave"], p["sample_rate"], _g(p["fmin"]), p["hop"], gamma,
                                                  _g(p["tuning"]), _g(p["filter_scale"]), _g(p["norm"]), window,
                                                  "true" if p["scale"] else "false", pad))


def frequencies(dtype, c: Config) -> np.ndarray:
    """``Cqt.frequencies dtype c`` (cqt.mli:243-255): the centre frequency of each bin in hertz."""
    out = np.empty(c.n_bins, dtype=np.float64)
    check(lib.smx_cqt_frequencies(c._h, C.c_void_p(out.ctypes.data)))
    return out.astype(dtype)


def filter_lengths(dtype, c: Config) -> np.ndarray:
    """``Cqt.filter_lengths dtype c`` (cqt.mli:257-269): the fractional support of each filter in samples at ``sample_rate``."""
    out = np.empty(c.n_bins, dtype=np.float64)
    check(lib.smx_cqt_filter_lengths(c._h, C.c_void_p(out.ctypes.data)))
    return out.astype(dtype)


def frames(c: Config, n: int) -> int:
    """``Cqt.frames c ~n`` (cqt.mli:278-281): the minimum over the octave plan of the octave's frame count."""
    count = C.c_int64()
    check(lib.smx_cqt_frames(c._h, int(n), C.byref(count)))
    return count.value


def _batch(fn, x):
    b = Batch(x, fn)
    if b.bytes != 4:
        raise _lib.InvalidArgument("%s: cannot analyse float64 audio (this path is float32)" % fn)
    return b


def _run(fn, c, x, complex_, host, device, params):
    b = _batch(fn, x)
    lead_shape, n = b.shape[:-1], int(b.shape[-1])
    lead = prod(lead_shape)
    return b.run(host, (c._h, b.ptr(), lead, n, *params, OUT), device, (c._h, b.ptr(), lead, n, max(n, 1), *params, OUT, STREAM),
                 lead_shape + (c.n_bins, frames(c, n)), complex_=complex_, null_empty=True)


def transform(c: Config, x):
    """``Cqt.transform cdtype c x`` (cqt.mli:285-303): ``[...; n]`` float32 -> ``[...; n_bins; frames]`` complex64."""
    return _run("transform", c, x, True, lib.smx_cqt_transform_f32, lib.smx_cqt_transform_f32_dev, ())


def power_spectrum(c: Config, x, power: float = 2.0):
    """``Cqt.power_spectrum ?power c x`` (cqt.mli:305-315): ``|transform c x| ^ power`` in float32, ``[...; n_bins; frames]``."""
    return _run("power_spectrum", c, x, False, lib.smx_cqt_power_spectrum_f32, lib.smx_cqt_power_spectrum_f32_dev, (float(power),))


# ---- Cqt.Kernel: the streaming transform (cqt.mli:317-413) ------------------------------------------------------------------

def _count(fn, *args) -> int:
    out = C.c_int64()
    check(fn(*args, C.byref(out)))
    return out.value


def columns_ready(c: Config, fed: int) -> int:
    """The columns a ``Kernel`` has returned once ``fed`` samples went in (cqt.mli:199-231): host arithmetic, no device.  A column
    leaves when every octave has projected it; for constant and edge padding that is ``max(0, (fed - latency) // hop + 1)``,
    under reflect an octave's frame 0 waits for one sample more (it reads the mirror of its first)."""
    return _count(lib.smx_cqt_config_columns_ready, c._h, int(fed))


def column_bound(c: Config, max_block: int) -> int:
    """The most columns one ``step`` of at most ``max_block`` samples, or ``flush``, returns."""
    return _count(lib.smx_cqt_config_column_bound, c._h, int(max_block))


def run_ahead(c: Config) -> int:
    """The most columns an octave can be ahead of the slowest one; the kernel's column ring holds ``run_ahead + column_bound``."""
    return _count(lib.smx_cqt_config_run_ahead, c._h)


class Kernel:
    """``Cqt.Kernel`` (cqt.ml:694-1012): ``prepare``, ``step``, ``flush``, ``reset``.  Chunks are float32 ``[...; m]`` whose leading
    axes multiply to ``channels``, host arrays or device tensors (then everything is enqueued on torch's current stream and
    nothing synchronises); ``step`` / ``flush`` return ``[...; n_bins; columns]`` complex64 -- float32 ``|z|^power`` when prepared
    with a ``power`` -- or ``None``.  Mutable, single-owner; the config outlives it."""

    def __init__(self, handle, c, channels, max_block, power):
        self._h, self._c, self.channels, self.max_block, self.power = handle, c, channels, max_block, power
        self._device, self._torch, self._lead = None, False, (channels,)

    @staticmethod
    def prepare(c: Config, channels: int, max_block: int, power=None) -> "Kernel":
        handle = C.c_void_p()
        check(lib.smx_cqt_kernel_prepare(c._h, int(channels), int(max_block), 0 if power is None else 1,
                                         2.0 if power is None else float(power), C.byref(handle)))
        return Kernel(handle, c, int(channels), int(max_block), None if power is None else float(power))

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h and lib is not None:
            try:
                lib.smx_cqt_kernel_destroy(h)
            except Exception:
                pass

    latency = property(lambda self: self._c.latency, doc="cqt.mli:196-231, in input samples")
    column_bound = property(lambda self: column_bound(self._c, self.max_block))

    def _empty(self, columns, device=None):
        shape = self._lead + (self._c.n_bins, columns)
        if device is not None:
            import torch
            return torch.empty(shape, dtype=torch.complex64 if self.power is None else torch.float32, device=device)
        return np.zeros(shape, dtype=np.complex64 if self.power is None else np.float32)

    def step(self, chunk):
        b = _batch("step", chunk)
        lead, m = b.shape[:-1], int(b.shape[-1])
        if prod(lead) != self.channels:
            raise _lib.InvalidArgument("step: cannot analyse %d channels (the kernel was prepared for %d)" % (prod(lead), self.channels))
        columns = max(0, lib.smx_cqt_kernel_columns_after(self._h, m))
        got = C.c_int64()
        self._lead, self._torch = lead, b.torch
        if b.device:
            self._device = b.data.device
            out = self._empty(columns, self._device) if columns else None
            with b.device_guard():
                check(lib.smx_cqt_kernel_step_f32_dev(self._h, b.ptr(), m, max(m, 1), out_ptr(out) if columns else None, columns,
                                                      C.byref(got), b.stream()))
            return out
        out = self._empty(columns) if columns else None
        check(lib.smx_cqt_kernel_step_f32(self._h, b.ptr(), m, max(m, 1), out_ptr(out) if columns else None, columns, C.byref(got)))
        return b.wrap(out) if columns else None

    def flush(self):
        """The withheld columns (None when there are none, and on a second flush); on the device if the stream was fed from it."""
        columns = max(0, lib.smx_cqt_kernel_pending(self._h))
        got = C.c_int64()
        if self._device is not None:
            import torch
            out = self._empty(columns, self._device) if columns else None
            with torch.cuda.device(self._device):
                stream = C.c_void_p(torch.cuda.current_stream(self._device).cuda_stream)
                check(lib.smx_cqt_kernel_flush_f32_dev(self._h, out_ptr(out) if columns else None, columns, C.byref(got), stream))
            return out
        out = self._empty(columns) if columns else None
        check(lib.smx_cqt_kernel_flush_f32(self._h, out_ptr(out) if columns else None, columns, C.byref(got)))
        if out is not None and self._torch:
            import torch
            return torch.from_numpy(out)
        return out

    def reset(self) -> None:
        self._device, self._torch = None, False
        check(lib.smx_cqt_kernel_reset(self._h))
