"""soundml_amd -- MI355X-native spectral path for SoundML (STFT / power
spectrogram, mel filterbank, FIR block convolution) behind the reference's own
module names:

    from soundml_amd import Stft, Mel, Chroma, Cqt, Hpss, Window, Fir, Resample, resample, mel_spectrogram, mfcc, chroma_stft, chroma_cqt, spectral_centroid
    from soundml_amd import rms, rms_of_spectrogram, rms_stage, zero_crossing_rate, zero_crossing_rate_stage
    from soundml_amd import Pitch, yin, yin_difference, yin_stage, pyin, pyin_observation, pyin_decode
    from soundml_amd import Rhythm, tempogram, tempo, beat_track
    from soundml_amd import Sequence, cost_matrix, dtw, dtw_distance
    from soundml_amd import Decompose, nmf, nmf_activations, nmf_reconstruct, nmf_divergence
    from soundml_amd import Iir                       # Iir.Config.create(sos), Iir.apply, Iir.filtfilt, Iir.zi, Iir.Kernel
    from soundml_amd import Loudness, loudness, true_peak      # BS.1770: Loudness.integrated / momentary / short_term / normalize / Meter
    from soundml_amd import Pcen, pcen                # per-channel energy normalisation: Pcen.Config.create, Pcen.apply / smooth / Kernel
    from soundml_amd import mel_to_stft, mel_to_audio, mfcc_to_mel, mfcc_to_audio      # and Mel.invert, Convert.db_to_power, ...

Everything computes in hand-written HIP kernels (gfx950) behind the C ABI of
``include/soundml_amd.h``; this package is the thin host mirror of
``Soundml.Stft`` / ``Soundml.Mel`` / ``Soundml.mel_spectrogram`` and fails loudly
if the HIP library is missing (no CPU fallback).
"""
from . import _lib
from ._lib import Failure, InvalidArgument, LIB_PATH, set_pinned_results, pinned_empty
from . import stft as Stft
from . import mel as Mel
from . import window as Window
from . import fir as Fir
from . import resample as Resample
from .resample import resample      # (the flat function takes the package attribute; the module is Resample)
from .resample import Spec
from . import chroma as Chroma
from . import cqt as Cqt
from . import convert as Convert
from .features import mel_spectrogram, mfcc, chroma_stft, chroma_cqt, power_to_db, amplitude_to_db
from .spectral import (spectral_centroid, spectral_bandwidth, spectral_rolloff, spectral_flatness,
                       spectral_centroid_stage, spectral_bandwidth_stage, spectral_rolloff_stage, spectral_flatness_stage)
from .contrast import spectral_contrast, spectral_contrast_of_spectrogram, spectral_contrast_stage
from .onset import onset_strength, onset_strength_stage
from .energy import rms, rms_of_spectrogram, rms_stage, zero_crossing_rate, zero_crossing_rate_stage
from . import pitch as Pitch
from .pitch import yin, yin_difference, yin_stage, pyin, pyin_observation, pyin_decode
from . import rhythm as Rhythm
from .rhythm import tempogram, tempo, beat_track
from . import sequence as Sequence
from .sequence import cost_matrix, dtw, dtw_distance
from . import decompose as Decompose
from .decompose import nmf, nmf_activations, nmf_reconstruct, nmf_divergence
from . import iir as Iir
from . import loudness as Loudness
from .loudness import integrated as loudness, true_peak      # (the flat function takes the package attribute; the module is Loudness)
from . import pcen as Pcen
from .pcen import pcen      # (the flat function takes the package attribute; the module is Pcen)
from . import hpss as Hpss
from .hpss import hpss_masks, hpss_of_spectrogram, hpss_of_stft, hpss, harmonic, percussive
from . import effects as Effects
from .effects import phase_vocoder, time_stretch, pitch_shift, semitones
from .inverse import mel_to_stft, mel_to_audio, mfcc_to_mel, mfcc_to_audio
from . import shard


def set_interior(name: str) -> None:
    """"float32" (default, fast) or "float64" (the reference's interior, stft.ml:28-35)."""
    _lib.check(_lib.lib.smx_set_interior(_lib.INTERIOR[name]))


def set_scratch_retention(nbytes: int) -> None:
    """Bytes of freed scratch the library keeps per device for reuse (-1: the default, 1/8 of device memory)."""
    _lib.check(_lib.lib.smx_set_scratch_retention(int(nbytes)))


def device_count() -> int:
    import ctypes
    n = ctypes.c_int()
    _lib.check(_lib.lib.smx_device_count(ctypes.byref(n)))
    return n.value


def set_devices(devices) -> None:
    """Clip sharding of the host-array batch calls over several GPUs from ONE process (the reference's caller is one process:
    stft.mli:211-250).  ``devices`` is a list of device ordinals (a device may appear more than once); ``Stft.transform`` /
    ``transform_range`` / ``power_spectrum`` / ``invert`` and ``mel_spectrogram`` on host arrays then split their leading
    axes into contiguous clip ranges (``shard.clip_range``), one host thread, staging ring pair and PCIe link per listed
    device, each writing its slice of the one result: bit-equal to the single-device call (stft_grid.ml:180-205).
    ``[]`` or ``None`` restores the single-device behaviour."""
    import ctypes
    ids = [int(d) for d in (devices or [])]
    arr = (ctypes.c_int * max(1, len(ids)))(*ids)
    _lib.check(_lib.lib.smx_set_devices(arr, len(ids)))


def get_devices():
    import ctypes
    n = ctypes.c_int()
    _lib.check(_lib.lib.smx_get_devices(None, 0, ctypes.byref(n)))
    arr = (ctypes.c_int * max(1, n.value))()
    _lib.check(_lib.lib.smx_get_devices(arr, n.value, ctypes.byref(n)))
    return [int(arr[i]) for i in range(n.value)]


__all__ = ["Stft", "Mel", "Chroma", "Cqt", "Convert", "Window", "Fir", "Resample", "resample", "Spec", "mel_spectrogram", "mfcc", "chroma_stft", "chroma_cqt", "power_to_db", "amplitude_to_db", "spectral_centroid",
           "spectral_bandwidth", "spectral_rolloff", "spectral_flatness", "spectral_contrast", "spectral_contrast_of_spectrogram", "spectral_contrast_stage", "onset_strength", "onset_strength_stage", "rms", "rms_of_spectrogram", "rms_stage", "zero_crossing_rate", "zero_crossing_rate_stage", "Pitch", "yin", "yin_difference", "yin_stage", "pyin", "pyin_observation", "pyin_decode", "Rhythm", "tempogram", "tempo", "beat_track", "Sequence", "cost_matrix", "dtw", "dtw_distance", "Decompose", "nmf", "nmf_activations", "nmf_reconstruct", "nmf_divergence", "Iir", "Loudness", "loudness", "true_peak", "Pcen", "pcen", "Hpss", "hpss_masks", "hpss_of_spectrogram", "hpss_of_stft", "hpss", "harmonic", "percussive", "Effects", "phase_vocoder", "time_stretch", "pitch_shift", "semitones", "mel_to_stft", "mel_to_audio", "mfcc_to_mel", "mfcc_to_audio", "shard", "set_interior", "set_pinned_results", "pinned_empty", "set_scratch_retention", "device_count", "set_devices", "get_devices",
           "InvalidArgument", "Failure", "LIB_PATH"]
