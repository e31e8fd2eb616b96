"""Audio to pitch contour on the device: a glide that falls silent and a tone that gives way to noise, tracked by pyin, next to
yin's raw frame-wise pitch on the same clips.

    python examples/pyin.py
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
truth = np.stack([110.0 * 2.0 ** (t / seconds), np.full_like(t, 220.0)])     # an octave up in three seconds; a steady tone
phase = 2 * np.pi * np.cumsum(truth, axis=-1) / rate
clips = np.sin(phase) + 0.5 * np.sin(2 * phase) + 0.25 * np.sin(3 * phase)
clips[0, 2 * rate:] = 0.0                                                   # the glide's last second is silence
clips[1, 2 * rate:] = 0.3 * rng.standard_normal(rate)                       # the tone's last second is noise
x = torch.from_numpy(clips.astype(np.float32)).cuda()                       # [2; n], resident

band = dict(fmin=65.0, fmax=2093.0, sample_rate=rate, frame_length=frame, hop=hop)
f0, voiced_flag, voiced_prob = [o[:, 0].cpu().numpy() for o in S.pyin(x, **band)]     # [2; frames] each
raw = S.yin(x, **band)[:, 0].cpu().numpy()
pmin, pmax = Pitch.lag_range(rate, 65.0, 2093.0, frame)
frames = f0.shape[-1]
centre = np.clip(np.arange(frames) * hop - frame // 2 + (frame // 2 + pmax) // 2, 0, t.size - 1)
sounding = np.arange(frames) * hop + frame // 2 < 2 * rate                  # frames that end before the third second
for k, name in enumerate(("glide, then silence", "tone, then noise")):
    voiced = voiced_flag[k] == 1.0
    inner = voiced & sounding & (np.arange(frames) > 3)
    cents = 1200.0 * np.abs(np.log2(f0[k, inner] / truth[k, centre[inner]]))
    print("%-20s %3d of %d frames voiced (%d of the %d that sound); f0 %.1f .. %.1f Hz, at most %.1f cents from the true pitch;"
          " unvoiced frames are %s" % (name, int(voiced.sum()), frames, int((voiced & sounding).sum()), int(sounding.sum()),
                                       np.nanmin(f0[k]), np.nanmax(f0[k]), cents.max(), "NaN" if np.isnan(f0[k, ~voiced]).all() else "mixed"))
    print("%-20s yin reports a pitch for every frame: %.1f .. %.1f Hz in the last second" % ("", raw[k, ~sounding].min(), raw[k, ~sounding].max()))

obs = S.pyin_observation(x, **band)                                          # [2; 2 n_bins; frames]
states = S.pyin_decode(obs, Pitch.pyin_half_width(rate, hop))                # [2; 1; frames]
n_bins = Pitch.pyin_bins(65.0, 2093.0)
print("pyin_observation: %s (%d pitch bins, voiced then unvoiced); pyin_decode of it: %s, %d frames in voiced states"
      % (tuple(obs.shape), n_bins, tuple(states.shape), int((states < n_bins).sum())))
