"""Onset strength of a click track over a tone, offline and as a stream of log-mel chunks.

    python examples/onset_strength.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import soundml_amd as S  # noqa: E402
from soundml_amd import Mel, Stft  # noqa: E402

rate, seconds, hop = 22050, 4, 512
t = np.arange(rate * seconds) / rate
x = 0.1 * np.sin(2 * np.pi * 220.0 * t)
x[::rate // 2] += 0.9                            # two clicks a second
x = x.astype(np.float32)

c = Stft.Config.create(fft_size=2048, hop=hop)
mc = Mel.Config.create(n_mels=128, sample_rate=rate, fft_size=2048)
envelope = S.onset_strength(c, mc, x, lag=1)    # [frames]; centred analysis is compensated by fft_size / (2 hop) frames
peaks = [i for i in range(1, len(envelope) - 1) if envelope[i] > 0.5 * envelope.max() and envelope[i] >= envelope[i - 1] and envelope[i] > envelope[i + 1]]
print("onsets at %s s (clicks every 0.5 s; shifted by %d frames = %.3f s)" % (
    ", ".join("%.2f" % (i * hop / rate) for i in peaks), 2048 // (2 * hop), 2048 // (2 * hop) * hop / rate))

# the same flux over chunks of a log-mel spectrogram: no clamp and no shift, one value per incoming frame
db = S.power_to_db(S.mel_spectrogram(c, mc, x))
stage = S.onset_strength_stage(lag=1)
streamed = np.concatenate([stage.step(db[:, a:a + 25]) for a in range(0, db.shape[-1], 25)])
print("streamed in chunks of 25 frames: %d values, equal to one chunk: %s" % (len(streamed), np.array_equal(streamed, S.onset_strength_stage(lag=1).step(db))))

contrast = S.spectral_contrast(c, x, sample_rate=rate)
print("spectral contrast %s: mean per band %s dB" % (contrast.shape, np.round(contrast.mean(axis=-1), 1)))
