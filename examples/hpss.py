"""Harmonic/percussive separation of a tone with clicks: two waveforms out, the spectra never leave the device.

    python examples/hpss.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from soundml_amd import Hpss, Stft  # noqa: E402

rate, seconds = 22050, 4
t = np.arange(rate * seconds) / rate
tone = 0.4 * np.sin(2 * np.pi * 440.0 * t) + 0.2 * np.sin(2 * np.pi * 660.0 * t)
clicks = np.zeros_like(tone)
clicks[::rate // 4] = 0.9                      # four clicks a second
x = (tone + clicks).astype(np.float32)

c = Stft.Config.create(fft_size=2048, hop=512)
harmonic, percussive = Hpss.hpss(c, x, kernel_size=(31, 31), power=2.0, margin=(1.0, 1.0))


def db(a, b):
    return 10 * np.log10(np.sum(a * a) / max(np.sum(b * b), 1e-30))


print("harmonic part:   %5.1f dB closer to the tone than to the clicks" % (db(harmonic, harmonic - tone) - db(harmonic, harmonic - clicks)))
print("percussive part: peak %.2f at the clicks, rms %.3f between them" % (np.abs(percussive[::rate // 4]).max(), np.sqrt(np.mean(percussive[100:rate // 4 - 100] ** 2))))
print("residual of the partition at unit margins: %.2e" % np.abs(harmonic + percussive - x).max())
