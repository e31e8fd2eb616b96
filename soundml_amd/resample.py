"""Resample: the overlap-save executor's pieces on the device.

The reference's planner / polyphase bank / cascade logic stay where they are (resample.ml); this mirrors the three
internal pieces a maintainer would route to the device: the OLS geometry, the prototype design, the block identity of
``soundml_resample_shape`` (resample_stubs.c:329-422) and one whole stage (``ols_run`` + drain) as a block convolution.

    proto = Resample.prototype(l=2, k=160, fc=0.45 / 2, beta=Fir.kaiser_beta(100.0))
    st = Resample.Stage.create(proto, l=2, m=1, k=160)
    y = Resample.Stage.apply(st, x)            # [...; n] -> [...; ceil(n L / M)]

and the front door (resample.mli:91-197), which designs the stage itself and runs any ratio:

    cfg = Resample.Config.create(44100, 16000)          # "fast" | "high" | "best" | Resample.Spec(attenuation, passband)
    y = Resample.apply(cfg, x)                          # = soundml_amd.resample(x, 44100, 16000)
    kern = Resample.Kernel.prepare(cfg, channels=2, max_block=4096)
"""
from __future__ import annotations

import ctypes as C
from collections import namedtuple

import numpy as np

from . import _lib
from ._lib import check, lib
from ._tensor import OUT, STREAM, Batch, out_ptr, prod


def ols_geom(rate: int, l: int, m: int, k: int):
    """resample.ml:292-300: (N, B, delta), or None when the stage is not OLS-eligible."""
    n, b, d, ok = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int()
    check(lib.smx_resample_ols_geom(int(rate), int(l), int(m), int(k), C.byref(n), C.byref(b), C.byref(d), C.byref(ok)))
    return (n.value, b.value, d.value) if ok.value else None


def prototype(l: int, k: int, fc: float, beta: float) -> np.ndarray:
    """resample.ml:145-163 `design_prototype`: 2 K L + 1 taps, float64, sum = L."""
    h = np.empty(2 * int(k) * int(l) + 1, dtype=np.float64)
    check(lib.smx_resample_prototype(int(l), int(k), float(fc), float(beta), C.c_void_p(h.ctypes.data)))
    return h


def shape(x: np.ndarray, h: np.ndarray, n: int, sl: int = 1, sm: int = 1) -> np.ndarray:
    """`soundml_resample_shape` (resample_stubs.c:329-422): complex128 half spectra [lines; n/2+1] -> [lines; w/2+1]."""
    x = np.ascontiguousarray(x, dtype=np.complex128)
    h = np.ascontiguousarray(h, dtype=np.complex128)
    lines = int(np.prod(x.shape[:-1])) if x.ndim > 1 else 1
    if n < 2 or n % 2 or sl < 1 or sm < 1 or (sl > 1 and sm > 1) or (sm > 1 and n % sm) or (n // sm if sm > 1 else n) < 2:
        raise _lib.Failure("soundml_resample_shape: invalid geometry")      # resample_stubs.c:383-389, checked first
    w = n * sl if sl > 1 else (n // sm if sm > 1 else n)
    if x.shape[-1] < n // 2 + 1 or h.shape[-1] < (w // 2 + 1 if sl > 1 else n // 2 + 1):
        raise _lib.Failure("soundml_resample_shape: buffer extents disagree")
    out = np.empty(x.shape[:-1] + (max(w, 0) // 2 + 1,), dtype=np.complex128)
    check(lib.smx_resample_shape_c128(C.c_void_p(x.ctypes.data), C.c_void_p(h.ctypes.data), C.c_void_p(out.ctypes.data),
                                      lines, int(n), int(sl), int(sm)))
    return out


class Stage:
    def __init__(self, handle, l, m, k):
        self._h, self.l, self.m, self.k = handle, l, m, k

    @staticmethod
    def create(proto, l: int, m: int, k: int) -> "Stage":
        proto = np.ascontiguousarray(np.asarray(proto, dtype=np.float64))
        if proto.shape != (2 * int(k) * int(l) + 1,):
            raise _lib.InvalidArgument("resample_stage_create: cannot use a %d-tap prototype for l = %d, k = %d (the "
                                       "prototype has 2 K L + 1 taps)" % (proto.shape[0], l, k))
        handle = C.c_void_p()
        check(lib.smx_resample_stage_create(C.c_void_p(proto.ctypes.data), int(l), int(m), int(k), C.byref(handle)))
        return Stage(handle, int(l), int(m), int(k))

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h and lib is not None:
            try:
                lib.smx_resample_stage_destroy(h)
            except Exception:
                pass

    def out_length(self, n: int) -> int:
        return lib.smx_resample_stage_out_length(self._h, int(n))

    @staticmethod
    def apply(st: "Stage", x):
        b = Batch(x, "resample_stage")
        if b.bytes != 4:
            raise _lib.InvalidArgument("resample_stage: cannot resample float64 audio (this path is float32)")
        n = int(b.shape[-1])
        lead = prod(b.shape[:-1])
        n_out = st.out_length(n)
        return b.run(lib.smx_resample_stage_apply_f32, (st._h, b.ptr(), lead, n, OUT),
                     lib.smx_resample_stage_apply_f32_dev, (st._h, b.ptr(), lead, n, n, OUT, n_out, STREAM), tuple(b.shape[:-1]) + (n_out,))


class Kernel:
    """``Resample.Kernel`` (resample.mli:270-319) of one pure xL or /M stage: ``prepare`` / ``step`` / ``flush`` / ``reset``.
    One state carries all channels; the block carry lives on the device.  ``step`` returns the newly computable samples
    ``[channels; k]`` or None (burst emission: whole block pairs), ``flush`` the tail or None; the concatenation of every
    step plus flush equals ``Stage.apply`` on the concatenated input bit for bit.  Host chunks give host arrays,
    device-resident (torch CUDA) chunks stay on the device."""

    def __init__(self, handle, stage, channels, max_block):
        self._h, self._stage, self.channels, self.max_block = handle, stage, channels, max_block

    @staticmethod
    def prepare(stage, channels: int, max_block: int):
        """``stage``: a ``Stage`` (one pure xL or /M stage) or a ``Config`` (any ratio: ``ConfigKernel``)."""
        if isinstance(stage, Config):
            return ConfigKernel.prepare(stage, channels, max_block)
        handle = C.c_void_p()
        check(lib.smx_resample_kernel_prepare(stage._h, int(channels), int(max_block), C.byref(handle)))
        return Kernel(handle, stage, int(channels), int(max_block))     # (the stage must outlive the kernel: held here)

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h and lib is not None:
            try:
                lib.smx_resample_kernel_destroy(h)
            except Exception:
                pass

    def reset(self) -> None:
        check(lib.smx_resample_kernel_reset(self._h))

    def _check(self, shape, what):
        lead = prod(shape[:-1]) if len(shape) > 1 else 1
        if len(shape) < 1 or lead != self.channels:      # resample.mli:309-311
            raise _lib.InvalidArgument("%s: cannot feed a chunk of shape %s to a kernel of %d channels (the leading axes must hold "
                                       "the channels)" % (what, tuple(shape), self.channels))

    def step(self, chunk):
        from ._tensor import is_device, is_torch
        self._check(tuple(chunk.shape), "step")
        n = int(chunk.shape[-1])
        got = C.c_int64()
        bound = max(1, lib.smx_resample_kernel_out_bound(self._h, n))
        if is_device(chunk):
            import torch
            x = chunk.to(torch.float32).reshape(self.channels, n).contiguous()
            out = torch.empty((self.channels, bound), device=chunk.device, dtype=torch.float32)
            with torch.cuda.device(chunk.device):
                stream = C.c_void_p(torch.cuda.current_stream(chunk.device).cuda_stream)
                check(lib.smx_resample_kernel_step_f32_dev(self._h, C.c_void_p(x.data_ptr()), n, max(n, 1), C.c_void_p(out.data_ptr()),
                                                           bound, C.byref(got), stream))
            return None if got.value == 0 else out[:, :got.value].contiguous()
        a = chunk.detach().cpu().numpy() if is_torch(chunk) else np.asarray(chunk)
        if a.dtype != np.float32:
            raise _lib.InvalidArgument("step: cannot resample float64 audio (this path is float32)")
        a = np.ascontiguousarray(a).reshape(self.channels, n)
        out = np.empty((self.channels, bound), dtype=np.float32)
        check(lib.smx_resample_kernel_step_f32(self._h, C.c_void_p(a.ctypes.data), n, max(n, 1), C.c_void_p(out.ctypes.data), bound,
                                               C.byref(got)))
        return None if got.value == 0 else np.ascontiguousarray(out[:, :got.value])

    def flush(self, device=None):
        """The delayed tail (None when there is none, and on a second flush).  ``device``: a torch device to receive it there."""
        got = C.c_int64()
        pending = lib.smx_resample_kernel_pending(self._h)
        cap = max(1, pending)
        if device is not None:
            import torch
            out = torch.empty((self.channels, cap), device=device, dtype=torch.float32)
            with torch.cuda.device(device):
                stream = C.c_void_p(torch.cuda.current_stream(device).cuda_stream)
                check(lib.smx_resample_kernel_flush_f32_dev(self._h, C.c_void_p(out.data_ptr()), cap, C.byref(got), stream))
            return None if got.value == 0 else out[:, :got.value].contiguous()
        out = np.empty((self.channels, cap), dtype=np.float32)
        check(lib.smx_resample_kernel_flush_f32(self._h, C.c_void_p(out.ctypes.data), cap, C.byref(got)))
        return None if got.value == 0 else np.ascontiguousarray(out[:, :got.value])


# ---- Resample.Config / Resample.apply: the one-call rate converter (resample.mli:91-197) ---------------------------------

Spec = namedtuple("Spec", ["attenuation", "passband"])
Spec.__doc__ = "The reference's `Custom {attenuation; passband}: stop-band rejection in dB, [40, 200]; kept band fraction, [0.5, 0.99]."

_QUALITY = {"fast": 0, "high": 1, "best": 2}
_EXECUTOR = {0: "identity", 1: "ols", 2: "direct"}


class _BorrowedStage(Stage):
    """The stage an "ols" config owns, seen as a ``Stage``: the config (held here) frees it."""

    def __init__(self, config):
        self._config = config
        self._h, self.l, self.m, self.k = C.c_void_p(lib.smx_resample_config_stage(config._h)), config.rate[0], config.rate[1], config.latency

    def __del__(self):      # borrowed: nothing to free
        self._h = None


class Config:
    """``Resample.Config`` (resample.mli:91-174, resample.ml:872-1151): the plan of a ``sample_rate`` -> ``target`` conversion.

    Creating one needs no device.  L / M = target / sample_rate reduced; L = M = 1 is the identity.  Otherwise ONE stage of the
    reference's single-stage design (resample.ml:919-932): ``latency`` K input samples, a ``2 K L + 1``-tap Kaiser prototype.

    DEVIATION from the reference's planner: every conversion is one stage.  ``executor`` is "ols" (the polyphase-block stage
    of ``Stage``) exactly for a pure x2..4 or /2..4 conversion that ``ols_geom`` reports eligible (resample.ml:951), "direct"
    (the polyphase dot product, 2 K + 1 multiply-adds per output) for everything else.  The reference's two-stage cascade
    search (``plan_cascade``, priced with constants measured on its own machine) is not restated: the ratios it cascades
    (48 <-> 8 kHz and the like) run the single-stage design its planner prices as ``cost_single`` -- the same spec, but a
    different ``latency`` -- and a ratio whose single-stage bank passes the 8 MiB budget raises even where a cascade would fit.
    """

    def __init__(self, handle, quality):
        self._h, self._quality = handle, quality

    @staticmethod
    def create(sample_rate: int, target: int, quality="high") -> "Config":
        if isinstance(quality, str):
            if quality not in _QUALITY:
                raise _lib.InvalidArgument("create: cannot use quality %r (one of 'fast', 'high', 'best', or a Resample.Spec)" % (quality,))
            kind, att, pb = _QUALITY[quality], 0.0, 0.0
        else:
            quality = Spec(float(quality[0]), float(quality[1]))
            kind, att, pb = 3, quality.attenuation, quality.passband
        handle = C.c_void_p()
        check(lib.smx_resample_config_create(int(sample_rate), int(target), kind, att, pb, C.byref(handle)))
        return Config(handle, quality)

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h and lib is not None:
            try:
                lib.smx_resample_config_destroy(h)
            except Exception:
                pass

    sample_rate = property(lambda self: lib.smx_resample_config_sample_rate(self._h))
    target = property(lambda self: lib.smx_resample_config_target(self._h))
    quality = property(lambda self: self._quality)
    rate = property(lambda self: (lib.smx_resample_config_l(self._h), lib.smx_resample_config_m(self._h)),
                    doc="(L, M): output samples per M input samples (resample.ml:1027)")
    latency = property(lambda self: lib.smx_resample_config_latency(self._h), doc="K, in input samples (resample.ml:1029)")
    executor = property(lambda self: _EXECUTOR[lib.smx_resample_config_executor(self._h)])

    @property
    def output_latency(self):
        """K L / M as a reduced (num, den), in output samples (resample.ml:1031-1036)."""
        num, den = C.c_int64(), C.c_int64()
        check(lib.smx_resample_config_output_latency(self._h, C.byref(num), C.byref(den)))
        return num.value, den.value

    @property
    def design(self):
        """(fc, beta) of the stage's Kaiser-sinc (resample.ml:931-932); (0, 0) for the identity."""
        fc, beta = C.c_double(), C.c_double()
        check(lib.smx_resample_config_design(self._h, C.byref(fc), C.byref(beta)))
        return fc.value, beta.value

    def output_frames(self, n: int) -> int:
        """ceil(n L / M) (resample.ml:1038-1051)."""
        out = C.c_int64()
        check(lib.smx_resample_config_output_frames(self._h, int(n), C.byref(out)))
        return out.value

    def prototype(self) -> np.ndarray:
        """A fresh float64 copy of the stage's prototype, 2 K L + 1 long (resample.ml:1053-1056)."""
        h = np.empty(lib.smx_resample_config_prototype_length(self._h), dtype=np.float64)
        check(lib.smx_resample_config_prototype(self._h, C.c_void_p(h.ctypes.data)))
        return h

    def __eq__(self, other):    # Config.equal (resample.ml:1139-1150): rates and quality; a Spec never equals a named quality
        if not isinstance(other, Config):
            return NotImplemented
        if (self.sample_rate, self.target) != (other.sample_rate, other.target):
            return False
        a, b = self._quality, other._quality
        if isinstance(a, str) or isinstance(b, str):
            return isinstance(a, str) and isinstance(b, str) and a == b
        return a.attenuation == b.attenuation and a.passband == b.passband

    def __hash__(self):
        return hash((self.sample_rate, self.target, self._quality))

    def __repr__(self):
        l, m = self.rate
        q = self._quality if isinstance(self._quality, str) else "custom(%g dB, %g)" % tuple(self._quality)
        return "resample(%d -> %d Hz, quality=%s, L/M=%d/%d, K=%d, executor=%s)" % (self.sample_rate, self.target, q, l, m,
                                                                                  self.latency, self.executor)


def apply(config: Config, x):
    """``Resample.apply`` (resample.mli:176-197): ``[...; n]`` -> ``[...; ceil(n L / M)]``, leading axes broadcast; the identity
    config returns ``x`` itself.  Host arrays give host arrays; a device-resident tensor is read through its strides where
    its leading axes flatten, and stays on the device.  float32 only (DEVIATION: the reference also takes float64)."""
    ex = config.executor
    shape = tuple(x.shape)
    if len(shape) < 1:   # resample.ml:66-70 check_rank
        raise _lib.InvalidArgument("apply: cannot resample a rank-zero tensor (the time axis must exist)")
    if ex == "identity":
        return x
    if ex == "ols":
        return Stage.apply(_BorrowedStage(config), x)
    n, lead = int(shape[-1]), prod(shape[:-1])
    n_out = config.output_frames(n)
    from ._tensor import is_device
    if is_device(x):
        import torch
        if x.dtype == torch.float64:
            raise _lib.InvalidArgument("apply: cannot resample float64 audio (this path is float32)")
        if x.dtype != torch.float32:
            x = x.to(torch.float32)
        stride = _row_stride(x)
        if stride is None:
            x = x.contiguous()
            stride = max(n, 1)
        out = torch.empty(shape[:-1] + (n_out,), dtype=torch.float32, device=x.device)
        with torch.cuda.device(x.device):
            stream = C.c_void_p(torch.cuda.current_stream(x.device).cuda_stream)
            check(lib.smx_resample_apply_f32_dev(config._h, C.c_void_p(x.data_ptr()), lead, n, stride, out_ptr(out), max(n_out, 1), stream))
        return out
    b = Batch(x, "apply")
    if b.bytes != 4:
        raise _lib.InvalidArgument("apply: cannot resample float64 audio (this path is float32)")
    out = b.empty(shape[:-1] + (n_out,))
    check(lib.smx_resample_apply_f32(config._h, b.ptr(), lead, n, out_ptr(out)))
    return b.wrap(out)


def _row_stride(x):
    """The one stride that walks every row of ``x`` viewed as [lead; n] (elements), or None where there is none."""
    shape, strides = tuple(x.shape), tuple(x.stride())
    n = shape[-1]
    if n > 1 and strides[-1] != 1:
        return None
    rows = [(d, s) for d, s in zip(shape[:-1], strides[:-1]) if d != 1]
    if not rows:
        return max(n, 1)
    step = rows[-1][1]
    expect = step
    for d, s in reversed(rows):     # the leading axes must flatten into one axis of that step
        if s != expect:
            return None
        expect = s * d
    return step if step >= max(n, 1) else None


def resample(x, sample_rate: int, target: int, quality="high"):
    """``Soundml.resample ~sample_rate ~target x``: ``apply`` on a config built for this call, as the reference's does."""
    return apply(Config.create(sample_rate, target, quality), x)


class ConfigKernel:
    """``Resample.Kernel`` (resample.mli:270-319) of a ``Config``.  "direct": the last 2 K samples of every channel stay on the
    device; after ``fed`` input samples in total the steps have emitted exactly ``max(0, ceil((fed - K) L / M))`` outputs
    (``ready``, resample.ml:1298), ``step`` returns None when that adds nothing, ``flush`` extends the signal with silence and
    emits up to ``ceil(total L / M)`` (None if nothing remains, and on a second flush), ``reset`` zeroes the history.  The
    concatenation of every step plus flush equals ``apply`` on the concatenated input bit for bit, under any chunking.
    An "ols" config prepares the block kernel of its stage (``Kernel``); the identity passes chunks through as copies."""

    def __init__(self, handle, config, channels, max_block):
        self._h, self._config, self.channels, self.max_block = handle, config, channels, max_block   # (the config outlives the kernel)
        self._drained = False

    @staticmethod
    def prepare(config: Config, channels: int, max_block: int):
        channels, max_block = int(channels), int(max_block)
        ex = config.executor
        if ex == "ols":
            stage = _BorrowedStage(config)
            handle = C.c_void_p()
            check(lib.smx_resample_kernel_prepare(stage._h, channels, max_block, C.byref(handle)))
            return Kernel(handle, stage, channels, max_block)
        if ex == "identity":
            if channels < 1 or max_block < 1:
                raise _lib.InvalidArgument("resample_kernel_prepare: cannot prepare a kernel for %d channels and chunks of %d samples "
                                           "(both must be at least 1)" % (channels, max_block))
            return ConfigKernel(None, config, channels, max_block)
        handle = C.c_void_p()
        check(lib.smx_resample_stream_prepare(config._h, channels, max_block, C.byref(handle)))
        return ConfigKernel(handle, config, channels, max_block)

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h and lib is not None:
            try:
                lib.smx_resample_stream_destroy(h)
            except Exception:
                pass

    def reset(self) -> None:
        self._drained = False
        if self._h:
            check(lib.smx_resample_stream_reset(self._h))

    _check = Kernel._check

    def _pass_through(self, chunk, n):
        if self._drained:
            raise _lib.InvalidArgument("resample_kernel_step: cannot feed a kernel drained by flush (reset it before a new signal)")
        if n > self.max_block:
            raise _lib.InvalidArgument("resample_kernel_step: cannot feed a chunk of %d samples to a kernel prepared for at most %d"
                                       % (n, self.max_block))
        if n == 0:
            return None
        from ._tensor import is_torch
        return chunk.clone() if is_torch(chunk) else np.array(chunk, copy=True)

    def step(self, chunk):
        from ._tensor import is_device, is_torch
        self._check(tuple(chunk.shape), "step")
        n = int(chunk.shape[-1])
        if not self._h:
            return self._pass_through(chunk, n)
        got = C.c_int64()
        bound = max(1, lib.smx_resample_stream_out_bound(self._h, n))
        if is_device(chunk):
            import torch
            x = chunk.to(torch.float32).reshape(self.channels, n).contiguous()
            out = torch.empty((self.channels, bound), device=chunk.device, dtype=torch.float32)
            with torch.cuda.device(chunk.device):
                stream = C.c_void_p(torch.cuda.current_stream(chunk.device).cuda_stream)
                check(lib.smx_resample_stream_step_f32_dev(self._h, C.c_void_p(x.data_ptr()), n, max(n, 1), C.c_void_p(out.data_ptr()),
                                                           bound, C.byref(got), stream))
            return None if got.value == 0 else out[:, :got.value].contiguous()
        a = chunk.detach().cpu().numpy() if is_torch(chunk) else np.asarray(chunk)
        if a.dtype != np.float32:
            raise _lib.InvalidArgument("step: cannot resample float64 audio (this path is float32)")
        a = np.ascontiguousarray(a).reshape(self.channels, n)
        out = np.empty((self.channels, bound), dtype=np.float32)
        check(lib.smx_resample_stream_step_f32(self._h, C.c_void_p(a.ctypes.data), n, max(n, 1), C.c_void_p(out.ctypes.data), bound,
                                               C.byref(got)))
        return None if got.value == 0 else np.ascontiguousarray(out[:, :got.value])

    def flush(self, device=None):
        """The delayed tail (None when there is none, and on a second flush).  ``device``: a torch device to receive it there."""
        if not self._h:
            self._drained = True
            return None
        got = C.c_int64()
        cap = max(1, lib.smx_resample_stream_pending(self._h))
        if device is not None:
            import torch
            out = torch.empty((self.channels, cap), device=device, dtype=torch.float32)
            with torch.cuda.device(device):
                stream = C.c_void_p(torch.cuda.current_stream(device).cuda_stream)
                check(lib.smx_resample_stream_flush_f32_dev(self._h, C.c_void_p(out.data_ptr()), cap, C.byref(got), stream))
            return None if got.value == 0 else out[:, :got.value].contiguous()
        out = np.empty((self.channels, cap), dtype=np.float32)
        check(lib.smx_resample_stream_flush_f32(self._h, C.c_void_p(out.ctypes.data), cap, C.byref(got)))
        return None if got.value == 0 else np.ascontiguousarray(out[:, :got.value])
