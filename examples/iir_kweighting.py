"""K-weighted loudness of a batch of resident clips: the two biquads of ITU-R BS.1770 at 48 kHz (the shelving pre-filter and the
RLB high-pass, coefficients as the recommendation prints them) in front of `rms`, all on the device.  A 1 kHz tone and a 50 Hz tone
of equal amplitude: the weighting leaves the first where it is (0 dB at 997 Hz plus the shelf's rise) and takes the hum down.

    python examples/iir_kweighting.py
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import soundml_amd as S  # noqa: E402
from soundml_amd import Iir  # noqa: E402

K_WEIGHTING_48K = np.array([
    # b0                b1                 b2                a0   a1                 a2
    [1.53512485958697, -2.69169618940638, 1.19839281085285, 1.0, -1.69065929318241, 0.73248077421585],     # stage 1: the head's shelf
    [1.0,              -2.0,              1.0,              1.0, -1.99004745483398, 0.99007225036621],     # stage 2: RLB high-pass
])

rate, seconds = 48000, 4
t = np.arange(rate * seconds) / rate
clips = np.stack([0.5 * np.sin(2 * np.pi * f * t) for f in (1000.0, 50.0)]).astype(np.float32)
x = torch.from_numpy(clips).cuda()                                  # [2; n], resident

c = Iir.Config.create(K_WEIGHTING_48K)
weighted = Iir.apply(c, x)                                          # [2; n], float32, still on the device
block, hop = rate * 400 // 1000, rate * 100 // 1000                 # BS.1770's 400 ms blocks, 75 % overlap
plain, kw = S.rms(x, frame_length=block, hop=hop)[:, 0], S.rms(weighted, frame_length=block, hop=hop)[:, 0]
mid = plain.shape[-1] // 2
for k, f in enumerate((1000, 50)):
    print("%4d Hz: rms %.4f, K-weighted %.4f (%+.2f dB), %.2f LKFS" % (
        f, float(plain[k, mid]), float(kw[k, mid]), 20 * np.log10(float(kw[k, mid]) / float(plain[k, mid])),
        -0.691 + 10 * np.log10(float(kw[k, mid]) ** 2)))

# the same signal as a stream of 4096-sample chunks, and filtered forward and backward for zero phase
k = Iir.Kernel.prepare(c, 2)
parts = [k.step(x[:, a:a + 4096]) for a in range(0, x.shape[-1], 4096)] + k.flush()
print("streamed in chunks of 4096 samples: equal to the flat call bit for bit: %s" % torch.equal(torch.cat(parts, dim=-1), weighted))
zero_phase = Iir.filtfilt(c, x)
lag = int(torch.argmax(weighted[0, rate:rate + 48])) - int(torch.argmax(zero_phase[0, rate:rate + 48]))
print("filtfilt: the weighting applied twice, no delay (the one-pass output's 1 kHz peaks lie %d samples from the zero-phase ones)" % lag)
