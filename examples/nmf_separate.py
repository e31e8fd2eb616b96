"""Take a clip apart into its notes: three notes played one after the other and then together, Stft.transform, nmf on |X| with
three components, Decompose.mask per component on the complex spectrum, Stft.invert -- nothing leaves the device until the
report at the end.

    python examples/nmf_separate.py
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import soundml_amd as S  # noqa: E402
from soundml_amd import Decompose, Stft  # noqa: E402

rate, seconds = 22050, 0.5
notes = [261.63, 329.63, 392.00]                                          # C, E, G
t = np.arange(int(rate * seconds)) / rate
tone = [sum(0.3 / h * np.sin(2 * np.pi * f * h * t) for h in (1, 2, 3)) * np.hanning(t.size) for f in notes]
clip = np.concatenate(tone + [tone[0] + tone[1] + tone[2]]).astype(np.float32)
x = torch.from_numpy(clip).cuda()                                         # [n], resident

c = Stft.Config.create(fft_size=2048, hop=512)
X = Stft.transform(c, x)                                                  # complex [1025; frames], resident
V = Stft.power_spectrum(c, x, power=1.0)                                  # |X|, resident
W, H = S.nmf(V, 3, n_iter=200, beta="kullback-leibler")                   # [1025; 3] templates, [3; frames] activations
print("objective %.4f after 200 rounds (from %.4f)" % (float(S.nmf_divergence(V, W, H, "kullback-leibler")),
                                                      float(S.nmf_divergence(V, *S.nmf(V, 3, n_iter=0), "kullback-leibler"))))
bins = np.fft.rfftfreq(2048, 1 / rate)
for k in range(3):
    y = Stft.invert(c, X * Decompose.mask(W, H, [k]), length=x.shape[-1])  # the component's share of the clip, resident
    peak = bins[int(torch.argmax(W[:, k]))]
    active = (H[k] > 0.5 * H[k].max()).float().mean()
    print("component %d: template peaks at %.0f Hz (notes at %s), active in %.0f %% of the frames, %.1f %% of the clip's energy" % (
        k, peak, ", ".join("%.0f" % f for f in notes), 100 * float(active), 100 * float((y ** 2).sum() / (x ** 2).sum())))
