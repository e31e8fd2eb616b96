"""Tensor plumbing between callers and the C ABI.

numpy arrays (and CPU torch tensors) take the host entry points of the library
(upload / run / download inside the C ABI, what an nx-tensor caller gets);
CUDA/HIP torch tensors take the device entry points on torch's current stream
and stay device-resident.  torch is only used for device memory and streams.

``Batch.run`` is the one dispatch between the two faces: a call site names its host pair and its device entry (the C ABI
spells the latter ``_f32_dev``, ``_dev_f32``, ``_device_f32``, ``_resident_f32``, ``_accel_f32``, ``_gpu_f32``, ``_hbm_f32``,
``_vram_f32`` or ``_card_f32``) with the arguments of each, and gets the outputs back in the caller's container.
``FramedStage`` is the one carry of the stages that frame a centred stream (``rms_stage``, ``yin_stage``, ...).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib

try:  # torch is optional plumbing: host-array callers never need it
    import torch
except Exception:  # pragma: no cover
    torch = None


def is_torch(x) -> bool:
    return torch is not None and isinstance(x, torch.Tensor)


def is_device(x) -> bool:
    return is_torch(x) and x.is_cuda


class Batch:
    """A real tensor viewed as [lead; n] (time axis last, leading axes flattened)."""

    def __init__(self, x, op: str, min_rank: int = 1, what: str = "analyse"):
        self.torch = is_torch(x)
        self.device = is_device(x)
        shape = tuple(x.shape)
        if len(shape) < min_rank:
            if min_rank == 1:   # stft.ml:289-293 check_rank
                raise _lib.InvalidArgument(
                    "%s: cannot analyse a rank-zero tensor (the time axis must exist)" % op)
        self.shape = shape
        self._ptr = None
        if self.device:
            if x.dtype not in (torch.float32, torch.float64):
                x = x.to(torch.float32)
            self.data = x.contiguous()
            self.bytes = 4 if self.data.dtype == torch.float32 else 8
        else:
            a = x.detach().cpu().numpy() if self.torch else np.asarray(x)
            if a.dtype not in (np.float32, np.float64):
                a = a.astype(np.float32)
            self.data = np.ascontiguousarray(a)
            self.bytes = self.data.dtype.itemsize

    def ptr(self):
        if self._ptr is None:
            self._ptr = C.c_void_p(self.data.data_ptr() if self.device else self.data.ctypes.data)
        return self._ptr

    def empty(self, shape, complex_=False, overwritten=False):
        """Fresh output tensor of the caller's kind; complex outputs get the
        matching complex dtype (stft.ml:681-685 spectrum_witness).  overwritten: the library
        writes every element (a large host result may then come from its page-locked pool)."""
        if self.device:
            if complex_:
                dt = torch.complex64 if self.bytes == 4 else torch.complex128
            else:
                dt = self.data.dtype
            return torch.empty(shape, dtype=dt, device=self.data.device)
        if complex_:
            dt = np.complex64 if self.bytes == 4 else np.complex128
        else:
            dt = self.data.dtype
        if overwritten:
            return _lib.host_result(shape, dt)
        return np.zeros(shape, dtype=dt)

    def wrap(self, out):
        """Return host results in the caller's container type."""
        if self.torch and not self.device:
            return torch.from_numpy(out)
        return out

    def zeros(self, shape):
        """Zeros of the caller's kind (``empty`` is uninitialised on the device)."""
        if self.device:
            return torch.zeros(shape, dtype=self.data.dtype, device=self.data.device)
        return self.wrap(np.zeros(shape, dtype=self.data.dtype))

    def stream(self):                                    # by index: torch converts a device object at ten times the cost
        return C.c_void_p(torch.cuda.current_stream(self.data.device.index).cuda_stream)

    def device_guard(self):
        return torch.cuda.device(self.data.device.index)

    def pick(self, entry):
        """An entry as it stands, or the one of its ``(_f32, _f64)`` pair for this tensor's width."""
        return entry if callable(entry) else entry[0] if self.bytes == 4 else entry[1]

    def run(self, host, host_args, device, device_args, shapes, *, skip=False, empty="zeros", prefill=False, null_empty=False,
            complex_=False, overwritten=False):
        """One library call on the face the tensor lies on.  ``host`` / ``device``: an entry, or its ``(_f32, _f64)`` pair;
        ``host_args`` / ``device_args``: that entry's arguments in its own order, with ``OUT`` where each output's pointer goes in
        turn and ``STREAM`` for torch's current stream (``self.ptr()`` is this tensor's pointer on either face).  ``shapes``: one
        output shape, or a list of them where ``None`` is an output not asked for (a null pointer, returned as ``None``);
        ``complex_`` / ``overwritten`` as in ``empty``, the latter also one flag per output.  Outputs come back in the caller's
        container, one or a tuple.

        ``skip``: the request is empty, no call is made and every output is ``empty``: "zeros", or "uninitialised" (what
        ``self.empty`` gives: zeros on the host, ``torch.empty`` on the device).  ``prefill``: device outputs are zeroed before
        the call.  ``null_empty``: a zero-size output is handed over as a null pointer."""
        single = type(shapes) is tuple
        if single:
            shapes = (shapes,)
        if skip:
            fresh = self.zeros if empty == "zeros" else lambda s: self.wrap(self.empty(s))
            outs = [None if s is None else fresh(s) for s in shapes]
            return outs[0] if single else tuple(outs)
        entry, args = (device, device_args) if self.device else (host, host_args)
        call, outs, at = list(args), [], -1
        for s in shapes:                                 # each output goes where the next ``OUT`` stands (the rest: numbers, ctypes)
            at = call.index(OUT, at + 1)
            o = None if s is None else self.empty(s, complex_, overwritten[len(outs)] if type(overwritten) is tuple else overwritten)
            call[at] = None if o is None or (null_empty and 0 in s) else out_ptr(o)
            outs.append(o)
        fn = self.pick(entry)
        if self.device:
            if prefill:
                for o in outs:
                    if o is not None and o.numel() > 0:
                        o.zero_()
            with self.device_guard():
                call[call.index(STREAM)] = self.stream()
                _lib.check(fn(*call))
        else:
            _lib.check(fn(*call))
            if self.torch:
                outs = [None if o is None else self.wrap(o) for o in outs]
        return outs[0] if single else tuple(outs)


class _Slot:
    def __init__(self, name):
        self._name = name

    def __repr__(self):
        return self._name


OUT, STREAM = _Slot("OUT"), _Slot("STREAM")          # the places of ``Batch.run``'s argument tuples


def refuse_device_float64(op, b, what="audio is"):
    if b.device and b.bytes != 4:
        raise _lib.Failure("%s: device-resident float64 %s not supported; pass a host array" % (op, what))


def out_ptr(out):
    if is_torch(out):
        return C.c_void_p(out.data_ptr())
    return C.c_void_p(out.ctypes.data)


def prod(shape) -> int:
    n = 1
    for d in shape:
        n *= int(d)
    return n


class Stateless:
    """``Pipeline.stateless f`` (the memoryless stage of the reference): every chunk maps through ``f`` on its own;
    nothing is withheld, so ``flush`` is empty and ``reset`` does nothing."""
    latency = 0

    def __init__(self, f):
        self._f = f

    def step(self, chunk):
        return self._f(chunk)

    __call__ = step

    def flush(self):
        return []

    def reset(self):
        pass


# ---- containers of a stage's carry: numpy, or torch on the chunk's device ---------------------------------------------------

def copy(t):
    return t.clone() if is_torch(t) else np.array(t)


def join(parts):
    return torch.cat(parts, dim=-1) if is_torch(parts[0]) else np.concatenate(parts, axis=-1)


def zeros_like_lead(t, width):
    shape = tuple(t.shape[:-1]) + (width,)
    if is_torch(t):
        return torch.zeros(shape, dtype=t.dtype, device=t.device)
    return np.zeros(shape, dtype=t.dtype)


def repeat(sample, width):
    """[...; 1] -> [...; width] copies"""
    if is_torch(sample):
        return sample.expand(tuple(sample.shape[:-1]) + (width,)).contiguous()
    return np.repeat(sample, width, axis=-1)


class FramedStage:
    """The streaming carry of a centred, framed analysis (energy.ml:194-347): the pending suffix of the padded stream (in the
    chunks' own container: numpy, or torch on the chunk's device), the last raw sample, and how many padded positions are still
    to drop when the hop outruns the data.  The left border (``frame_length // 2`` "zeros", or "edge" copies of the first
    sample) installs with the first non-empty chunk, ``flush`` appends the right one; every call hands ``pending ++ chunk`` to
    ``_segment`` for exactly the frames that became complete.  Only shapes decide the control flow: device chunks cause no
    synchronisation."""

    def __init__(self, name: str, frame_length: int, hop: int, border: str):
        self.name, self.frame_length, self.hop = name, int(frame_length), int(hop)
        self._pad = {"zeros": zeros_like_lead, "edge": repeat}[border]
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

    def _segment(self, samples, count):
        """frames [0, count) of a segment of the padded stream"""
        raise NotImplementedError

    def _process(self, extra, borrowed):
        """energy.ml:232-259: ``extra`` joins the pending stream; the frames that became complete are emitted."""
        parts = ([] if self._pending is None else [self._pending]) + extra
        fresh = len(parts) > 1 or not borrowed
        samples = parts[0] if len(parts) == 1 else join(parts)
        total = int(samples.shape[-1])
        fl, hop = self.frame_length, self.hop
        count = 0 if total < fl else 1 + (total - fl) // hop
        if count == 0:
            self._pending = samples if fresh else copy(samples)
            return None
        out = self._segment(samples, count)
        next_start = count * hop
        if next_start >= total:
            self._skip += next_start - total
            self._pending = None
        else:
            self._pending = copy(samples[..., next_start:])
        return out

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
        refuse_device_float64(self.name, b)
        chunk = b.data if b.device or not b.torch else b.wrap(b.data)   # float32 / float64, contiguous, the caller's container
        self._tail = copy(chunk[..., m - 1:])
        if not self._started:
            self._started = True
            if self.border == 0:
                return self._process([chunk], True)
            return self._process([self._pad(chunk[..., :1], self.border), chunk], True)
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
            right = self._pad(self._tail, self.border)
            if self._skip >= self.border:
                self._skip -= self.border
            else:
                dropped, self._skip = self._skip, 0
                out = self._process([right[..., dropped:] if dropped else right], False)
        self._pending = None
        return [] if out is None else [out]
