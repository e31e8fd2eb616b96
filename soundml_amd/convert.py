"""``Soundml.Convert`` (convert.ml): the decibel conversions (device) and the scalar maps (host values).

    Convert.power_to_db(s, top_db=80.0)          # see features.power_to_db
    Convert.db_to_power(db, reference=1.0)       # reference * 10 ** (db / 10), any shape, host or device
    Convert.hz_to_mel(f, scale="slaney")         # float64 host values, shape preserved
    Convert.hz_to_midi(f)                        # the same for MIDI numbers
    Convert.frames_to_time(22050, 512, frames)   # frame indices <-> seconds on a hop grid
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import check, lib
from ._tensor import OUT, STREAM, Batch, prod
from .features import amplitude_to_db, power_to_db  # noqa: F401


def _from_db(which, db, reference):
    if not hasattr(db, "shape"):
        db = np.asarray(db)
    b = Batch(db, which, min_rank=0)
    total = prod(b.shape)
    entries = [getattr(lib, "smx_%s_%s" % (which, sfx)) for sfx in ("f32", "f64", "f32_dev", "f64_dev")]
    args = (b.ptr(), total, float(reference), OUT)
    return b.run(entries[:2], args, entries[2:], args + (STREAM,), b.shape)


def db_to_power(db, reference: float = 1.0):
    """``Convert.db_to_power ?reference db`` (convert.ml:58-64): reference * 10 ** (db / 10) in db's own dtype,
    evaluated in float64 and rounded once."""
    return _from_db("db_to_power", db, reference)


def db_to_amplitude(db, reference: float = 1.0):
    """``Convert.db_to_amplitude ?reference db`` (convert.ml:66-68): reference * 10 ** (db / 20)."""
    return _from_db("db_to_amplitude", db, reference)


def _host_map(call, values):
    """A float64 host map with the input's shape and float dtype."""
    v = np.ascontiguousarray(np.asarray(values, dtype=np.float64))
    out = np.empty_like(v)
    check(call(C.c_void_p(v.ctypes.data), int(v.size), C.c_void_p(out.ctypes.data)))
    src = np.asarray(values)
    return out.astype(src.dtype) if src.dtype in (np.float32, np.float64) else out


def _scale_map(fn, values, scale):
    if scale not in _lib.MEL_SCALE:
        raise _lib.InvalidArgument("%s: unknown mel scale %r" % (fn.__name__, scale))
    return _host_map(lambda v, n, out: fn(_lib.MEL_SCALE[scale], v, n, out), values)


def hz_to_mel(f, scale: str = "slaney"):
    """``Convert.hz_to_mel ?scale f`` (convert.ml:80-90)."""
    return _scale_map(lib.smx_hz_to_mel, f, scale)


def mel_to_hz(m, scale: str = "slaney"):
    """``Convert.mel_to_hz ?scale m`` (convert.ml:92-102)."""
    return _scale_map(lib.smx_mel_to_hz, m, scale)


def hz_to_midi(f):
    """``Convert.hz_to_midi f`` (convert.ml:104): 12 log2 (f / 440) + 69."""
    return _host_map(lib.smx_hz_to_midi, f)


def midi_to_hz(m):
    """``Convert.midi_to_hz m`` (convert.ml:106): 440 * 2 ** ((m - 69) / 12)."""
    return _host_map(lib.smx_midi_to_hz, m)


def frames_to_time(sample_rate: int, hop: int, frames):
    """``Convert.frames_to_time ~sample_rate ~hop frames`` (convert.ml:108-110): frames * hop / sample_rate seconds."""
    return _host_map(lambda v, n, out: lib.smx_frames_to_time(int(sample_rate), int(hop), v, n, out), frames)


def time_to_frames(sample_rate: int, hop: int, times):
    """``Convert.time_to_frames ~sample_rate ~hop times`` (convert.ml:112-115): floor (times * sample_rate / hop)."""
    return _host_map(lambda v, n, out: lib.smx_time_to_frames(int(sample_rate), int(hop), v, n, out), times)
