"""Frame energy and zero-crossing rate of a batch of resident clips, next to their onset strength, with a silence gate as the
use: frames whose rms lies 40 dB under the clip's loudest frame carry no onsets worth keeping.

    python examples/energy.py
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import soundml_amd as S  # noqa: E402
from soundml_amd import Mel, Stft  # noqa: E402

rate, seconds, fft, hop = 22050, 4, 2048, 512
t = np.arange(rate * seconds) / rate
rng = np.random.default_rng(0)
clips = np.stack([0.3 * np.sin(2 * np.pi * f * t) for f in (220.0, 440.0, 880.0)])
clips[:, : rate] = 0.0                                             # a second of silence first ...
clips[:, 3 * rate:] = 1e-4 * rng.standard_normal((3, rate))        # ... and a second of faint noise last
clips[:, rate::rate // 2] += 0.9                                   # two clicks a second from then on
x = torch.from_numpy(clips.astype(np.float32)).cuda()              # [3; n], resident

c = Stft.Config.create(fft_size=fft, hop=hop)
mc = Mel.Config.create(n_mels=128, sample_rate=rate, fft_size=fft)
energy = S.rms(x, frame_length=fft, hop=hop)[:, 0]                 # [3; frames], on the STFT's centred frame grid
crossings = S.zero_crossing_rate(x, frame_length=fft, hop=hop)[:, 0]
onsets = S.onset_strength(c, mc, x)                                # [3; frames]
assert energy.shape == crossings.shape == onsets.shape

loud = energy > energy.amax(dim=-1, keepdim=True) * 10.0 ** (-40.0 / 20.0)
gated = torch.where(loud, onsets, torch.zeros_like(onsets))
for k in range(3):
    print("clip %d: %3d of %d frames above the gate; onset strength kept %.1f of %.1f; the tone crosses zero %.4f per sample (2 f / rate = %.4f), the noise %.2f"
          % (k, int(loud[k].sum()), loud.shape[-1], float(gated[k].sum()), float(onsets[k].sum()),
             float(crossings[k, 60]), 2 * (220.0 * 2 ** k) / rate, float(crossings[k, -10])))

# the same energy from the magnitude spectrogram of a rectangular window (Parseval), and as a stream of 4096-sample chunks
r = Stft.Config.create(fft_size=fft, hop=hop, window="rectangular", pad=("constant", 0.0))
spectral = S.rms_of_spectrogram(Stft.power_spectrum(r, x, 1.0), frame_length=fft)[:, 0]
print("rms_of_spectrogram against rms: max difference %.2e" % float((spectral - energy).abs().max()))
stage = S.rms_stage(frame_length=fft, hop=hop)
parts = [stage.step(x[:, a:a + 4096]) for a in range(0, x.shape[-1], 4096)] + stage.flush()
streamed = torch.cat([p for p in parts if p is not None], dim=-1)[:, 0]
print("streamed in chunks of 4096 samples: equal to the flat call bit for bit: %s" % torch.equal(streamed, energy))
