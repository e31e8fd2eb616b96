"""Shift a tone up a major third and stretch it to 1.25 times its length: the spectra never leave the device.

    python examples/pitch_shift.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from soundml_amd import Effects, Stft  # noqa: E402

rate, seconds = 22050, 2
t = np.arange(rate * seconds) / rate
x = (0.5 * np.sin(2 * np.pi * 440.0 * t)).astype(np.float32)

c = Stft.Config.create(fft_size=2048, hop=512)
ratio = Effects.semitones(4)                       # (349, 277): 2 ** (4 / 12) within 0.027 cents
shifted = Effects.pitch_shift(c, x, ratio, phase="locked")
slower = Effects.time_stretch(c, x, rate=0.8)


def peak_hz(y):
    spectrum = np.abs(np.fft.rfft(y[4096:-4096] * np.hanning(y.shape[0] - 8192)))
    return float(np.argmax(spectrum)) * rate / (y.shape[0] - 8192)


print("ratio %d/%d: the 440 Hz tone now peaks at %.1f Hz (equal temperament: %.1f Hz), length %d -> %d"
      % (ratio[0], ratio[1], peak_hz(shifted), 440.0 * 2 ** (4 / 12), x.shape[0], shifted.shape[0]))
print("rate 0.8: length %d -> %d, still peaking at %.1f Hz" % (x.shape[0], slower.shape[0], peak_hz(slower)))
