"""Pitch on MI355X: YIN fundamental-frequency tracking (de Cheveigne & Kawahara 2002), exported flat as ``yin`` /
``yin_difference`` / ``yin_stage``, and pYIN on top of it, ``pyin`` / ``pyin_observation`` / ``pyin_decode``.  The
reference has no such module; the parameters carry the usual names.

    f0 = yin(x, fmin=65, fmax=2093, sample_rate=22050)                     # [...; n] -> [...; 1; frames]
    f0, ap = yin(x, 65, 2093, return_aperiodicity=True)                    # the voicing measure d'(tau) next to it
    d = yin_difference(x, 65, 2093)                                        # [...; n] -> [...; pmax + 1; frames]
    stage = yin_stage(65, 2093)                                            # audio chunks [...; m] -> [...; 1; k] | None; flush() -> list
    f0, voiced_flag, voiced_prob = pyin(x, 65, 2093)                       # pYIN (Mauch & Dixon 2014): [...; n] -> three [...; 1; frames]
    obs = pyin_observation(x, 65, 2093)                                    # [...; n] -> [...; 2 n_bins; frames]
    states = pyin_decode(obs, pyin_half_width())                           # [...; 2 n_bins; frames] -> [...; 1; frames]

The frame grid is that of ``rms``: the signal is centred by ``frame_length // 2`` virtual zeros on each side and frames advance
by ``hop`` (``frame_length // 4`` when ``None``).  Float64 inside, one rounding to the dtype of the input.  The correlation and the
energies of a frame have one summation order, a function of its own samples, so a leading slice of a batch, a
range of frames and any chunking of the stage give the flat call's values bit for bit (include/soundml_amd.h words the
definition).
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from ._lib import InvalidArgument, check, lib
from ._tensor import OUT, STREAM, Batch, FramedStage, prod, refuse_device_float64
from .energy import frames       # noqa: F401  (the grid is rms')


def _hop(frame_length, hop):
    return int(frame_length) // 4 if hop is None else int(hop)


def lag_range(sample_rate: int, fmin: float, fmax: float, frame_length: int = 2048):
    """(pmin, pmax): the lags searched, ``floor(sample_rate / fmax)`` to ``ceil(sample_rate / fmin)``, the latter capped at
    ``frame_length - frame_length // 2 - 1``; the ABI checks the parameters and words what is wrong with them."""
    sr, fl, fmin, fmax = int(sample_rate), int(frame_length), float(fmin), float(fmax)
    check(lib.smx_yin_difference_f32(None, 0, 0, sr, fmin, fmax, fl, 1, None))
    longest, cap = sr / fmin, fl - fl // 2 - 1
    return int(math.floor(sr / fmax)), cap if longest >= cap else int(math.ceil(longest))


def _batch(name, x, fl, hop):
    b = Batch(x, name)
    refuse_device_float64(name, b)
    n = int(b.shape[-1])
    return b, n, b.shape[:-1], prod(b.shape[:-1]), frames(n, fl, hop)


def _run(name, x, params, count_of, host, resident, want_ap):
    """one frame call: the parameters are checked before the tensor is looked at"""
    b = Batch(x, name)
    refuse_device_float64(name, b)
    n = int(b.shape[-1])
    lead = prod(b.shape[:-1])
    count = count_of(n)
    shape = b.shape[:-1] + (1, count)
    f0, ap = b.run(host, (b.ptr(), lead, n, *params, OUT, OUT), resident, (b.ptr(), lead, n, n, *params, OUT, OUT, STREAM),
                   [shape, shape if want_ap else None], skip=lead == 0 or count == 0)
    return (f0, ap) if want_ap else f0


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
    return _run("yin", x, params, lambda n: frames(n, fl, hop), (lib.smx_yin_f32, lib.smx_yin_f64), lib.smx_yin_resident_f32,
                bool(return_aperiodicity))


def yin_difference(x, fmin: float, fmax: float, sample_rate: int = 22050, frame_length: int = 2048, hop=None):
    """The cumulative-mean-normalised difference d'(tau), tau = 0 .. pmax, of every frame: [...; n] -> [...; pmax + 1; frames]
    (``lag_range`` gives pmax)."""
    name = "yin_difference"
    fl, hop = int(frame_length), _hop(frame_length, hop)
    params = (int(sample_rate), float(fmin), float(fmax), fl, hop)
    check(lib.smx_yin_difference_f32(None, 0, 0, *params, None))
    lags = lag_range(sample_rate, fmin, fmax, fl)[1] + 1
    b, n, lead_shape, lead, count = _batch(name, x, fl, hop)
    return b.run((lib.smx_yin_difference_f32, lib.smx_yin_difference_f64), (b.ptr(), lead, n, *params, OUT),
                 lib.smx_yin_difference_resident_f32, (b.ptr(), lead, n, n, *params, OUT, STREAM), lead_shape + (lags, count),
                 skip=lead == 0 or count == 0)


def segment_frames(samples, count: int, fmin: float, fmax: float, sample_rate: int = 22050, frame_length: int = 2048, hop=None,
                   trough_threshold: float = 0.1, return_aperiodicity: bool = False):
    """Frames [0, count) of a segment of the padded stream, no border: the stage's body.  [...; n] -> [...; 1; count];
    (count - 1) * hop + frame_length <= n."""
    fl, hop, count = int(frame_length), _hop(frame_length, hop), int(count)
    params = (count, int(sample_rate), float(fmin), float(fmax), fl, hop, float(trough_threshold))
    check(lib.smx_yin_frames_f32(None, 0, 0, 0, *params[1:], None, None))
    return _run("yin_stage", samples, params, lambda n: count, (lib.smx_yin_frames_f32, lib.smx_yin_frames_f64),
                lib.smx_yin_frames_resident_f32, bool(return_aperiodicity))


class YinStage(FramedStage):
    """The streaming form of ``yin``: the framed-stream carry (the pending suffix of the padded stream, the skip when the hop
    outruns the data) with zero borders, as rms', over this module's segment call.  Only shapes decide the control flow: device
    chunks cause no synchronisation.  A step returns [...; 1; k], a pair with ``return_aperiodicity``, or None."""

    def __init__(self, fmin: float, fmax: float, sample_rate: int = 22050, frame_length: int = 2048, hop=None,
                 trough_threshold: float = 0.1, return_aperiodicity: bool = False):
        self.threshold = float(trough_threshold)
        self.fmin, self.fmax, self.sample_rate = float(fmin), float(fmax), int(sample_rate)
        self.return_aperiodicity = bool(return_aperiodicity)
        check(lib.smx_yin_frames_f32(None, 0, 0, 0, self.sample_rate, self.fmin, self.fmax, int(frame_length), _hop(frame_length, hop),
                                     self.threshold, None, None))
        super().__init__("yin_stage", frame_length, _hop(frame_length, hop), "zeros")

    def _segment(self, samples, count):
        return segment_frames(samples, count, self.fmin, self.fmax, self.sample_rate, self.frame_length, self.hop, self.threshold,
                              self.return_aperiodicity)


def yin_stage(fmin: float, fmax: float, sample_rate: int = 22050, frame_length: int = 2048, hop=None, trough_threshold: float = 0.1,
              return_aperiodicity: bool = False):
    """``yin`` over a stream of chunks: ``step`` / ``flush`` / ``reset``, latency ``frame_length // 2``, rate ``(1, hop)``."""
    return YinStage(fmin, fmax, sample_rate, frame_length, hop, trough_threshold, return_aperiodicity)


# ---- pYIN (Mauch & Dixon 2014): probabilistic YIN with Viterbi decoding; DESIGN.md 4.8j, include/soundml_amd.h words the definition.
# The decoder sees the whole clip before it answers: it is offline by definition and has no streaming stage.
OBSERVATION_FLOOR = 2.0 ** -200          # the least observation probability the decoder uses: keeps a path alive across a jump wider than the band


def _pyin_params(fmin, fmax, sample_rate, frame_length, hop, n_thresholds, beta_parameters, boltzmann_parameter, resolution,
                 max_transition_rate, switch_prob, no_trough_prob):
    a, b = beta_parameters
    return (int(sample_rate), float(fmin), float(fmax), int(frame_length), _hop(frame_length, hop), int(n_thresholds), float(a), float(b),
            float(boltzmann_parameter), float(resolution), float(max_transition_rate), float(switch_prob), float(no_trough_prob))


def pyin_bins(fmin: float, fmax: float, resolution: float = 0.1) -> int:
    """The pitch bins between ``fmin`` and ``fmax``: ``floor(12 bps log2(fmax / fmin)) + 1`` with ``bps = ceil(1 / resolution)``."""
    n = C.c_int64()
    check(lib.smx_pyin_bins(float(fmin), float(fmax), float(resolution), C.byref(n)))
    return int(n.value)


def pyin_half_width(sample_rate: int = 22050, hop: int = 512, resolution: float = 0.1, max_transition_rate: float = 35.92) -> int:
    """h, the half-width of the transition band in bins: ``(m bps) // 2`` with ``m`` the semitones a pitch may move per frame,
    ``max_transition_rate * 12 * hop / sample_rate`` rounded half to even."""
    h = C.c_int64()
    check(lib.smx_pyin_half_width(int(sample_rate), int(hop), float(resolution), float(max_transition_rate), C.byref(h)))
    return int(h.value)


def pyin_tables(fmin: float, fmax: float, sample_rate: int = 22050, frame_length: int = 2048, hop=None, n_thresholds: int = 100,
                beta_parameters=(2, 18), boltzmann_parameter: float = 2.0, resolution: float = 0.1, max_transition_rate: float = 35.92,
                switch_prob: float = 0.01, no_trough_prob: float = 0.01):
    """The host tables of the definition as float64 numpy arrays: ``thr`` [n + 1], ``beta`` [n], ``E`` [maxr], ``Z`` [maxr + 1]
    (``Z[0]`` = 0), ``freq`` [n_bins], ``edge`` [n_bins - 1] (b = 1 ..), ``tri`` [2 h + 1], ``rs`` [n_bins]; also ``n_bins``, ``h`` and
    ``maxr``, the most troughs a frame can have."""
    params = _pyin_params(fmin, fmax, sample_rate, frame_length, hop, n_thresholds, beta_parameters, boltzmann_parameter, resolution,
                          max_transition_rate, switch_prob, no_trough_prob)
    check(lib.smx_pyin_tables(*params, *([None] * 8)))
    pmin, pmax = lag_range(sample_rate, fmin, fmax, int(frame_length))
    n, maxr = params[5], (pmax - pmin) // 2 + 1
    n_bins, h = pyin_bins(fmin, fmax, resolution), pyin_half_width(sample_rate, params[4], resolution, max_transition_rate)
    sizes = dict(thr=n + 1, beta=n, E=maxr, Z=maxr + 1, freq=n_bins, edge=n_bins - 1, tri=2 * h + 1, rs=n_bins)
    out = {k: np.zeros(v, np.float64) for k, v in sizes.items()}
    check(lib.smx_pyin_tables(*params, *(out[k].ctypes.data for k in sizes)))
    out.update(n_bins=n_bins, h=h, maxr=maxr)
    return out




def pyin(x, fmin: float, fmax: float, sample_rate: int = 22050, frame_length: int = 2048, hop=None, n_thresholds: int = 100,
         beta_parameters=(2, 18), boltzmann_parameter: float = 2.0, resolution: float = 0.1, max_transition_rate: float = 35.92,
         switch_prob: float = 0.01, no_trough_prob: float = 0.01, fill_na=float("nan")):
    """Probabilistic YIN [...; n] -> ``(f0, voiced_flag, voiced_prob)``, each [...; 1; frames]: every trough of yin's d' is a pitch
    candidate weighted over ``n_thresholds`` thresholds with a beta prior, the candidates are binned ``resolution`` semitones apart
    and a Viterbi decoder picks one track through voiced and unvoiced states whose pitch moves at most ``max_transition_rate``
    octaves per second.  ``voiced_flag`` is a 1.0 / 0.0 mask in the dtype of the input, ``f0`` is ``fill_na`` on unvoiced frames
    (the bin's frequency with ``fill_na=None``); a frame that holds a non-finite sample has a NaN ``voiced_prob``.  Offline by
    definition: there is no streaming stage."""
    name = "pyin"
    params = _pyin_params(fmin, fmax, sample_rate, frame_length, hop, n_thresholds, beta_parameters, boltzmann_parameter, resolution,
                          max_transition_rate, switch_prob, no_trough_prob)
    fill = (1, 0.0) if fill_na is None else (0, float(fill_na))
    check(lib.smx_pyin_f32(None, 0, 0, *params, *fill, None, None, None))
    b, n, lead_shape, lead, count = _batch(name, x, params[3], params[4])
    return b.run((lib.smx_pyin_f32, lib.smx_pyin_f64), (b.ptr(), lead, n, *params, *fill, OUT, OUT, OUT),
                 lib.smx_pyin_accel_f32, (b.ptr(), lead, n, n, *params, *fill, OUT, OUT, OUT, STREAM), [lead_shape + (1, count)] * 3,
                 skip=lead == 0 or count == 0)


def pyin_observation(x, fmin: float, fmax: float, sample_rate: int = 22050, frame_length: int = 2048, hop=None, n_thresholds: int = 100,
                     beta_parameters=(2, 18), boltzmann_parameter: float = 2.0, resolution: float = 0.1,
                     max_transition_rate: float = 35.92, switch_prob: float = 0.01, no_trough_prob: float = 0.01):
    """The decoder's input [...; n] -> [...; 2 n_bins; frames]: the probability of every voiced pitch bin, then
    ``(1 - voiced_prob) / n_bins`` on every unvoiced one; NaN columns where a frame holds a non-finite sample."""
    name = "pyin_observation"
    params = _pyin_params(fmin, fmax, sample_rate, frame_length, hop, n_thresholds, beta_parameters, boltzmann_parameter, resolution,
                          max_transition_rate, switch_prob, no_trough_prob)
    check(lib.smx_pyin_observation_f32(None, 0, 0, *params, None))
    states = 2 * pyin_bins(fmin, fmax, resolution)
    b, n, lead_shape, lead, count = _batch(name, x, params[3], params[4])
    return b.run((lib.smx_pyin_observation_f32, lib.smx_pyin_observation_f64), (b.ptr(), lead, n, *params, OUT),
                 lib.smx_pyin_observation_accel_f32, (b.ptr(), lead, n, n, *params, OUT, STREAM), lead_shape + (states, count),
                 skip=lead == 0 or count == 0)


def pyin_decode(obs, half_width: int, switch_prob: float = 0.01):
    """The most probable state sequence of an observation [...; 2 n_bins; frames] -> [...; 1; frames], exact integers in the dtype
    of the input: state ``s < n_bins`` is voiced bin ``s``, ``n_bins + b`` unvoiced bin ``b``.  A pitch moves at most
    ``half_width`` bins per frame (``pyin_half_width``); observations below ``OBSERVATION_FLOOR`` count as the floor."""
    name = "pyin_decode"
    h, sp = int(half_width), float(switch_prob)
    check(lib.smx_pyin_decode_f32(None, 0, 0, 0, h, sp, None))
    b = Batch(obs, name)
    refuse_device_float64(name, b, "observations are")
    if len(b.shape) < 2:
        raise InvalidArgument("%s: cannot decode a tensor of rank %d (the state and frame axes must exist)" % (name, len(b.shape)))
    states, count = int(b.shape[-2]), int(b.shape[-1])
    lead_shape = b.shape[:-2]
    lead = prod(lead_shape)
    skip = lead == 0 or count == 0
    if skip:
        check(lib.smx_pyin_decode_f32(None, lead, states, count, h, sp, None))
    return b.run((lib.smx_pyin_decode_f32, lib.smx_pyin_decode_f64), (b.ptr(), lead, states, count, h, sp, OUT),
                 lib.smx_pyin_decode_accel_f32, (b.ptr(), lead, states, count, states * count, h, sp, OUT, STREAM), lead_shape + (1, count),
                 skip=skip)
