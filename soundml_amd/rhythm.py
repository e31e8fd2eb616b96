"""Rhythm on MI355X: the autocorrelation tempogram (Grosche, Mueller & Kurth 2010), the tempo under a log-normal prior and the
dynamic-programming beat tracker (Ellis 2007), exported flat as ``tempogram`` / ``tempo`` / ``beat_track``.  The reference has no
such module; the parameters carry the usual names.

    env = onset_strength(sc, mc, x)                                        # [...; frames], and it stays on the device
    tg = tempogram(env)                                                    # [...; frames] -> [...; win_length; frames]
    bpm = tempo(env, sample_rate=22050, hop=512)                           # [...; 1]
    bpm, beats = beat_track(env, sample_rate=22050, hop=512)               # [...; 1] and a 1.0 / 0.0 mask [...; frames]
    frames = Rhythm.beat_frames(beats)                                     # index arrays on the host (synchronises)

Float64 inside, one rounding to the dtype of the input.  Every sum has one order, a function of the clip's own values
(include/soundml_amd.h words the definitions), so a leading slice of a batch gives the batch's slice bit for bit.
Device tensors run on the caller's stream and nothing synchronises; float64 on the device is refused.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib, window as Window
from ._lib import check, lib
from ._tensor import OUT, STREAM, Batch, prod, refuse_device_float64


def _window(name, kind):
    try:
        family, param = Window.family(kind)
    except _lib.InvalidArgument as e:
        raise _lib.InvalidArgument("%s: %s" % (name, str(e).split(": ", 1)[1])) from None
    return _lib.WINDOW[family], 0.0 if param is None else param


def _batch(name, env):
    b = Batch(env, name)
    refuse_device_float64(name, b, "envelopes are")
    return b, int(b.shape[-1]), b.shape[:-1], prod(b.shape[:-1])


def tempogram(env, win_length: int = 384, window="hann", norm: bool = True):
    """The autocorrelation tempogram [...; frames] -> [...; win_length; frames]: row ``tau`` of frame ``t`` is the autocorrelation
    at lag ``tau`` of the ``win_length`` envelope values around ``t`` under ``Window.make``'s periodic window, divided by the
    value at lag 0 with ``norm``.  The envelope is extended by ``win_length // 2`` ZEROS on the left and the rest of the window on
    the right, as ``rms`` extends its signal, not by librosa's linear ramp: the first and the last ``win_length // 2`` frames
    differ from librosa's."""
    name = "tempogram"
    W = int(win_length)
    kind, param = _window(name, window)
    params = (W, kind, param, 1 if norm else 0)
    check(lib.smx_rhythm_tempogram_f32(None, 0, 0, *params, None))
    b, frames, lead_shape, lead = _batch(name, env)
    return b.run((lib.smx_rhythm_tempogram_f32, lib.smx_rhythm_tempogram_f64), (b.ptr(), lead, frames, *params, OUT),
                 lib.smx_rhythm_tempogram_gpu_f32, (b.ptr(), lead, frames, frames, *params, OUT, STREAM), lead_shape + (W, frames),
                 skip=lead == 0 or frames == 0, overwritten=True)


def _tempo(name, env, sample_rate, hop, win_length, start_bpm, std_bpm, max_tempo, want_lag):
    params = (int(sample_rate), int(hop), int(win_length), float(start_bpm), float(std_bpm), float(max_tempo), want_lag)
    check(lib.smx_rhythm_tempo_f32(None, 0, 0, *params, None))
    b, frames, lead_shape, lead = _batch(name, env)
    return b.run((lib.smx_rhythm_tempo_f32, lib.smx_rhythm_tempo_f64), (b.ptr(), lead, frames, *params, OUT),
                 lib.smx_rhythm_tempo_gpu_f32, (b.ptr(), lead, frames, frames, *params, OUT, STREAM), lead_shape + (1,), skip=lead == 0)


def tempo(env, sample_rate: int = 22050, hop: int = 512, win_length: int = 384, start_bpm: float = 120.0, std_bpm: float = 1.0,
          max_tempo: float = 320.0):
    """One tempo per clip in beats per minute, [...; frames] -> [...; 1]: the lag at which the frame mean of the normalised
    tempogram (hann window), weighted by a log-normal prior around ``start_bpm`` that is ``std_bpm`` octaves wide, is greatest,
    among the lags at or below ``max_tempo``.  NaN for an envelope that is empty or holds a non-finite value."""
    return _tempo("tempo", env, sample_rate, hop, win_length, start_bpm, std_bpm, max_tempo, 0)


def tempo_lag(env, sample_rate: int = 22050, hop: int = 512, win_length: int = 384, start_bpm: float = 120.0, std_bpm: float = 1.0,
              max_tempo: float = 320.0):
    """The lag ``tempo`` chooses, as [...; 1] in the dtype of the input: ``tempo`` is ``tempo_frequencies(..)[lag]``."""
    return _tempo("tempo", env, sample_rate, hop, win_length, start_bpm, std_bpm, max_tempo, 1)


def tempo_frequencies(win_length: int = 384, sample_rate: int = 22050, hop: int = 512) -> np.ndarray:
    """bpm of the lags 0 .. win_length - 1 in float64: ``60 * sample_rate / (hop * lag)``, infinite at lag 0."""
    out = np.empty(max(int(win_length), 1), np.float64)
    check(lib.smx_rhythm_tempo_frequencies(int(win_length), int(sample_rate), int(hop), C.c_void_p(out.ctypes.data)))
    return out[:int(win_length)]


def tempo_prior(win_length: int = 384, sample_rate: int = 22050, hop: int = 512, start_bpm: float = 120.0, std_bpm: float = 1.0,
                max_tempo: float = 320.0) -> np.ndarray:
    """The library's own table of ``-0.5 * ((log2 bpm(lag) - log2 start_bpm) / std_bpm) ** 2`` in float64, ``-inf`` at lag 0 and
    above ``max_tempo``."""
    out = np.empty(max(int(win_length), 1), np.float64)
    check(lib.smx_rhythm_tempo_prior(int(win_length), int(sample_rate), int(hop), float(start_bpm), float(std_bpm), float(max_tempo),
                                     C.c_void_p(out.ctypes.data)))
    return out[:int(win_length)]


def beat_period(bpm: float, sample_rate: int = 22050, hop: int = 512) -> int:
    """Frames per beat at ``bpm``: ``round_half_even(60 * sample_rate / hop / bpm)``, at least 1 and at most 4096."""
    p = C.c_int64()
    check(lib.smx_rhythm_beat_period(int(sample_rate), int(hop), float(bpm), C.byref(p)))
    return int(p.value)


def beat_tables(period: int, tightness: float = 100.0):
    """(g, tx): the library's own float64 tables of the tracker for one period, ``g(k) = exp(-0.5 * (32 k / period) ** 2)`` for
    ``k = -period .. period`` and ``tx(k) = -tightness * log(-w_k / period) ** 2`` for ``w = -2 period .. -round_half_even(period / 2)``."""
    p = int(period)
    check(lib.smx_rhythm_beat_tables(p, float(tightness), None, None))
    half = p // 2 + ((p // 2) & 1 if p & 1 else 0)
    g, tx = np.empty(2 * p + 1, np.float64), np.empty(2 * p - half + 1, np.float64)
    check(lib.smx_rhythm_beat_tables(p, float(tightness), C.c_void_p(g.ctypes.data), C.c_void_p(tx.ctypes.data)))
    return g, tx


def beat_track(env, sample_rate: int = 22050, hop: int = 512, bpm=None, win_length: int = 384, start_bpm: float = 120.0,
               tightness: float = 100.0, trim: bool = True):
    """Beat positions by dynamic programming, [...; frames] -> (tempo [...; 1], beats [...; frames]); ``beats`` is 1.0 at a beat
    frame and 0.0 elsewhere (``beat_frames`` lists them).  The beat period is the lag ``tempo`` chooses, or that of ``bpm`` when
    given; ``tightness`` weighs steadiness of the tempo against the onsets, ``trim`` drops weak leading and trailing beats.  A
    clip that is constant, shorter than 2 frames or not finite has no beats; clips of more than 8192 frames are refused."""
    name = "beat_track"
    has = bpm is not None
    params = (int(sample_rate), int(hop), 1 if has else 0, float(bpm) if has else 0.0, int(win_length), float(start_bpm), float(tightness),
              1 if trim else 0)
    check(lib.smx_rhythm_beat_track_f32(None, 0, 0, *params, None, None))
    b, frames, lead_shape, lead = _batch(name, env)
    return b.run((lib.smx_rhythm_beat_track_f32, lib.smx_rhythm_beat_track_f64), (b.ptr(), lead, frames, *params, OUT, OUT),
                 lib.smx_rhythm_beat_track_gpu_f32, (b.ptr(), lead, frames, frames, *params, OUT, OUT, STREAM),
                 [lead_shape + (1,), lead_shape + (frames,)], skip=lead == 0)


def beat_frames(beats):
    """The beat frames of a mask [...; frames] as int64 index arrays on the host: one array for a single clip, nested lists of
    arrays along the leading axes otherwise.  A device mask is copied to the host, which SYNCHRONISES its stream."""
    a = beats.detach().cpu().numpy() if hasattr(beats, "detach") else np.asarray(beats)

    def walk(m):
        return np.flatnonzero(m) if m.ndim == 1 else [walk(r) for r in m]
    return walk(a)
