"""The way back from the features: mel spectrogram or MFCC matrix -> magnitudes -> audio.

    s = mel_to_stft(mel_config, m)                      # [...; n_mels; frames] -> [...; bins; frames] magnitudes
    x = mel_to_audio(stft_config, mel_config, m)        # ... -> Stft.griffin_lim -> [...; n]
    m = mfcc_to_mel(c, n_mels=128)                      # [...; n_mfcc; frames] -> [...; n_mels; frames] powers
    x = mfcc_to_audio(stft_config, mel_config, c)

The reference has no inverse of ``Mel.apply``; the solver is ``Mel.invert`` (DESIGN.md "Mel inversion"), ``mfcc_to_mel``
is the tail of ``Soundml.mfcc`` (soundml.ml:26-95) backwards.  A device tensor stays on the device from end to end.
"""
from __future__ import annotations

from . import _lib
from ._lib import check, lib
from ._tensor import OUT, STREAM, Batch, prod
from . import mel as Mel
from . import stft as Stft


def mel_to_stft(mel_config, m, power: float = 2.0, n_iter: int = 200):
    """``Mel.invert mel_config m ** (1 / power)``: the magnitudes behind a mel spectrogram of |X| ** power.  The root is
    taken in float64 where the solver stores its result (power 2: a square root), rounded once to m's dtype."""
    return Mel._invert(mel_config, m, n_iter, power)


def _check_fft_sizes(fn, stft_config, mel_config):
    if stft_config.fft_size != mel_config.fft_size:
        raise _lib.InvalidArgument(
            "%s: cannot project a %d-point STFT through a filterbank built for an FFT of "
            "size %d (the two configurations must agree on fft_size)"
            % (fn, stft_config.fft_size, mel_config.fft_size))


def mel_to_audio(stft_config, mel_config, m, power: float = 2.0, n_iter: int = 200, gl_iter: int = 32,
                 momentum: float = 0.99, init=None, length=None):
    """``Stft.griffin_lim stft_config (mel_to_stft mel_config m)``: a signal whose mel spectrogram approaches m."""
    _check_fft_sizes("mel_to_audio", stft_config, mel_config)
    return Stft.griffin_lim(stft_config, mel_to_stft(mel_config, m, power, n_iter), gl_iter, momentum, init, length)


def mfcc_to_mel(c, n_mels: int, lifter=None, reference: float = 1.0):
    """The tail of ``Soundml.mfcc`` backwards: row k divided by its lifter weight, the cepstral axis zero-padded to
    ``n_mels``, the inverse orthonormal DCT-II along it, then ``db_to_power(., reference)``; float64 inside, one rounding.
    [...; n_mfcc; frames] -> [...; n_mels; frames] in c's dtype."""
    nd = len(c.shape)
    if nd < 2:
        raise _lib.InvalidArgument(
            "mfcc_to_mel: cannot invert a rank-%d tensor (the cepstral and frame axes must exist)" % nd)
    b = Batch(c, "mfcc_to_mel")
    lead_shape = b.shape[:-2]
    n_mfcc, frames = int(b.shape[-2]), int(b.shape[-1])
    lead = prod(lead_shape)
    has_lifter = lifter is not None
    tail = (int(n_mels), 1 if has_lifter else 0, float(lifter) if has_lifter else 0.0, float(reference))
    host = (lib.smx_mfcc_to_mel_f32, lib.smx_mfcc_to_mel_f64)
    check(b.pick(host)(None, 0, n_mfcc, 0, *tail, None))   # the checks first
    args = (b.ptr(), lead, n_mfcc, frames, *tail, OUT)
    return b.run(host, args, (lib.smx_mfcc_to_mel_f32_dev, lib.smx_mfcc_to_mel_f64_dev), args + (STREAM,),
                 lead_shape + (int(n_mels), frames))


def mfcc_to_audio(stft_config, mel_config, c, lifter=None, reference: float = 1.0, power: float = 2.0, n_iter: int = 200,
                  gl_iter: int = 32, momentum: float = 0.99, init=None, length=None):
    """``mel_to_audio stft_config mel_config (mfcc_to_mel c)``, the mel axis being the filterbank's."""
    _check_fft_sizes("mfcc_to_audio", stft_config, mel_config)
    m = mfcc_to_mel(c, mel_config.n_mels, lifter, reference)
    return mel_to_audio(stft_config, mel_config, m, power, n_iter, gl_iter, momentum, init, length)
