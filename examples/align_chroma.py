"""Align a melody with a slower performance of itself: chroma_cqt of a synthetic clip and of its Effects.time_stretch at rate 0.8,
then dtw on the pair without the features leaving the device; Sequence.warping_path is the only copy to the host.

    python examples/align_chroma.py
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import soundml_amd as S  # noqa: E402
from soundml_amd import Cqt, Effects, Sequence, Stft  # noqa: E402

rate, note_seconds, stretch = 22050, 0.4, 0.8
scale = [261.63, 293.66, 329.63, 349.23, 392.00, 440.00, 493.88, 523.25]                   # C major, up and down again
t = np.arange(int(rate * note_seconds)) / rate
clip = np.concatenate([0.5 * np.sin(2 * np.pi * f * t) * np.hanning(t.size) for f in scale + scale[::-1]]).astype(np.float32)
x = torch.from_numpy(clip).cuda()                                         # [n], resident
y = Effects.time_stretch(Stft.Config.create(fft_size=2048, hop=512), x, rate=stretch)      # the slower performance, resident

c = Cqt.Config.create(n_bins=84, sample_rate=rate)
cx, cy = S.chroma_cqt(c, x), S.chroma_cqt(c, y)                           # [12; n] and [12; m], resident
D, path = S.dtw(cx, cy)                                                   # [n; m] and [2; n + m - 1], resident
cells = Sequence.warping_path(path)                                       # the host copy: int64 [L; 2]
slope = np.polyfit(cells[:, 0], cells[:, 1], 1)[0]
print("chroma %s against %s: a path of %d cells, total cost %.3f" % (tuple(cx.shape), tuple(cy.shape), len(cells), float(S.dtw_distance(cx, cy))))
print("fitted slope of the path %.3f; the stretch was 1 / %.1f = %.3f" % (slope, stretch, 1 / stretch))
