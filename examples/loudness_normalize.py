"""Loudness normalisation of a batch of resident clips (ITU-R BS.1770-4): stereo clips at mixed levels brought to -23 LUFS under a
-1 dBTP true-peak ceiling without leaving the device, and the same clip metered as a stream of 4096-sample chunks.

    python examples/loudness_normalize.py
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from soundml_amd import Convert, Loudness  # noqa: E402

rate, seconds = 48000, 10
rng = np.random.default_rng(0)
t = np.arange(rate * seconds) / rate
levels = (-6.0, -20.0, -35.0, -50.0)                                # dBFS of a 1 kHz tone with some noise on top, per clip
clips = np.stack([10.0 ** (db / 20.0) * (np.stack([np.sin(2 * np.pi * 1000.0 * t), np.sin(2 * np.pi * 1000.0 * t + 0.5)])
                                         + 0.1 * rng.standard_normal((2, t.size))) for db in levels]).astype(np.float32)
x = torch.from_numpy(clips).cuda()                                  # [4; 2; n], resident

ceiling = 10.0 ** (-1.0 / 20.0)                                     # -1 dBTP as a linear amplitude
y = Loudness.normalize(x, rate, target=-23.0, peak_ceiling=ceiling)
before, after = Loudness.integrated(x, rate), Loudness.integrated(y, rate)
peak = Convert.amplitude_to_db(Loudness.true_peak(y).amax(-1), top_db=None)
for k, db in enumerate(levels):
    print("clip at %5.1f dBFS: %6.2f LUFS -> %6.2f LUFS, true peak %5.2f dBTP" % (db, float(before[k]), float(after[k]), float(peak[k])))

# the first clip as a stream: momentary loudness as blocks complete, the running integrated and short-term loudness at the end
meter = Loudness.Meter.prepare(rate, 2)
parts = [meter.step(x[0, :, a:a + 4096]) for a in range(0, x.shape[-1], 4096)]
momentary = torch.cat([p for p in parts if p is not None], dim=-1)
print("streamed in chunks of 4096 samples: %d momentary values, equal to the flat call bit for bit: %s" % (
    momentary.shape[-1], torch.equal(momentary, Loudness.momentary(x[0], rate))))
print("integrated %.2f LUFS (flat call: %.2f), last short-term value %.2f LUFS" % (
    float(meter.integrated()), float(before[0]), float(meter.short_term()[-1])))
