"""Tempo and beats of a click track: audio -> onset_strength -> beat_track, all resident; Rhythm.beat_frames is the only copy to
the host.

    python examples/beat_track.py
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import soundml_amd as S  # noqa: E402
from soundml_amd import Mel, Rhythm, Stft  # noqa: E402

rate, seconds, hop, bpm = 22050, 12, 512, 112.0
t = np.arange(rate * seconds) / rate
clips = np.stack([0.1 * np.sin(2 * np.pi * 220.0 * t), 0.1 * np.sin(2 * np.pi * 330.0 * t)])
starts = [np.arange(0.25, seconds, 60.0 / bpm), np.arange(0.40, seconds, 60.0 / 90.0)]      # a clip at 112 and one at 90 beats per minute
for row, at in zip(clips, starts):
    for s in at:
        i = int(round(s * rate))
        row[i:i + 64] += 0.9 * np.hanning(64)
x = torch.from_numpy(clips.astype(np.float32)).cuda()                      # [2; n], resident

sc = Stft.Config.create(fft_size=2048, hop=hop)
mc = Mel.Config.create(n_mels=128, sample_rate=rate, fft_size=2048)
envelope = S.onset_strength(sc, mc, x)                                     # [2; frames], resident
tempo, beats = S.beat_track(envelope, sample_rate=rate, hop=hop)           # [2; 1] and the 1.0 / 0.0 mask [2; frames], resident
tempi = tempo[:, 0].tolist()
for k, frames in enumerate(Rhythm.beat_frames(beats)):                     # the host copy
    times = frames * hop / rate
    print("clip %d: %.1f beats per minute (clicks at %.1f); %d beats, the first at %s s, %.3f s apart on average"
          % (k, tempi[k], (bpm, 90.0)[k], len(times), ", ".join("%.2f" % s for s in times[:4]), float(np.diff(times).mean()) if len(times) > 1 else 0.0))
print("tempogram of the envelopes: %s" % (tuple(S.tempogram(envelope).shape),))
