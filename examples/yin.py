"""The pitch of a batch of resident clips: a glide, a vibrato and a tone that gives way to noise, tracked by yin, with the
aperiodicity as the voicing gate, and the same track from a stream of chunks.

    python examples/yin.py
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import soundml_amd as S  # noqa: E402
from soundml_amd import Pitch  # noqa: E402

rate, seconds, frame, hop = 22050, 3, 2048, 512
t = np.arange(rate * seconds) / rate
rng = np.random.default_rng(0)
glide = 110.0 * 2.0 ** (t / seconds)                                      # an octave up in three seconds
vibrato = 440.0 * (1.0 + 0.01 * np.sin(2 * np.pi * 5.0 * t))
truth = np.stack([glide, vibrato, np.full_like(t, 220.0)])
phase = 2 * np.pi * np.cumsum(truth, axis=-1) / rate
clips = np.sin(phase) + 0.5 * np.sin(2 * phase) + 0.25 * np.sin(3 * phase)
clips[2, 2 * rate:] = 0.3 * rng.standard_normal(rate)                     # the last second of the third clip is noise
x = torch.from_numpy(clips.astype(np.float32)).cuda()                     # [3; n], resident

f0, aperiodicity = S.yin(x, fmin=65.0, fmax=2093.0, sample_rate=rate, frame_length=frame, hop=hop, return_aperiodicity=True)
f0, aperiodicity = f0[:, 0].cpu().numpy(), aperiodicity[:, 0].cpu().numpy()   # [3; frames]
voiced = aperiodicity < 0.1
# a frame reads its first W + pmax samples; compare with the true frequency at the middle of that span
pmin, pmax = Pitch.lag_range(rate, 65.0, 2093.0, frame)
centre = np.clip(np.arange(f0.shape[-1]) * hop - frame // 2 + (frame // 2 + pmax) // 2, 0, t.size - 1)
for k, name in enumerate(("glide", "vibrato", "tone, then noise")):
    ok = voiced[k] & (np.arange(f0.shape[-1]) > 3) & (np.arange(f0.shape[-1]) < f0.shape[-1] - 3)
    err = np.abs(f0[k, ok] / truth[k, centre[ok]] - 1.0)
    print("%-17s %3d of %d frames voiced; f0 %.1f .. %.1f Hz; worst deviation from the true pitch %.2f%%"
          % (name, int(voiced[k].sum()), voiced.shape[-1], f0[k, ok].min(), f0[k, ok].max(), 100 * err.max()))

d = S.yin_difference(x, 65.0, 2093.0, sample_rate=rate, frame_length=frame, hop=hop)       # [3; pmax + 1; frames]
print("yin_difference: %s, lags %d .. %d searched; the least d' of the glide's middle frame lies at lag %d (%.1f Hz)"
      % (tuple(d.shape), pmin, pmax, int(d[0, pmin:, d.shape[-1] // 2].argmin()) + pmin,
         rate / (int(d[0, pmin:, d.shape[-1] // 2].argmin()) + pmin)))

stage = S.yin_stage(65.0, 2093.0, sample_rate=rate, frame_length=frame, hop=hop)
parts = [stage.step(x[:, a:a + 4096]) for a in range(0, x.shape[-1], 4096)] + stage.flush()
streamed = torch.cat([p for p in parts if p is not None], dim=-1)[:, 0].cpu().numpy()
print("streamed in chunks of 4096 samples: equal to the flat call bit for bit: %s" % np.array_equal(streamed, f0))
