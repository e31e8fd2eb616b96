"""Per-channel energy normalisation of a batch of resident clips, offline and as a stream.  Offline: `pcen` from audio in one call (the
mel spectrogram never leaves the device).  Streaming: the same clips through `Stft.Kernel` (power 1), the mel filterbank and
`Pcen.Kernel` in chunks of 4096 samples; the frames that come out equal the offline result bit for bit.

    python examples/pcen.py
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import soundml_amd as S  # noqa: E402
from soundml_amd import Mel, Pcen, Stft  # noqa: E402

rate, seconds, fft, hop, n_mels = 22050, 4, 2048, 512, 128
t = np.arange(rate * seconds) / rate
rng = np.random.default_rng(0)
# a quiet and a loud take of the same chirp over noise: PCEN's gain control brings them together where log-mel keeps them 40 dB apart
chirp = np.sin(2 * np.pi * (200.0 + 400.0 * t) * t) * (t > 1.0) + 0.05 * rng.standard_normal(t.size)
clips = np.stack([0.01 * chirp, 1.0 * chirp]).astype(np.float32)
x = torch.from_numpy(clips).cuda()                                  # [2; n], resident

sc = Stft.Config.create(fft_size=fft, hop=hop)
mc = Mel.Config.create(n_mels=n_mels, sample_rate=rate, fft_size=fft)
c = Pcen.Config.create(sr=rate, hop=hop, scale=2.0 ** 31)           # librosa's convention for float audio
P = S.pcen(sc, mc, x, c)                                            # [2; n_mels; frames], float32, still on the device
mel = S.mel_spectrogram(sc, mc, x, power=1.0)
print("pcen from audio: %s, smoothing coefficient %.5f" % (tuple(P.shape), c.coefficient))
print("equal to Pcen.apply of the mel spectrogram bit for bit: %s" % torch.equal(P, Pcen.apply(c, mel)))
late = slice(P.shape[-1] // 2, None)
print("quiet against loud take, mean over the second half: log-mel %.1f dB apart, pcen %.2f against %.2f" % (
    float(10 * torch.log10(mel[1, :, late].mean() / mel[0, :, late].mean())), float(P[0, :, late].mean()), float(P[1, :, late].mean())))

# the same clips as a stream of host chunks: magnitude frames as they complete (Stft.Kernel behind Stft.power_stage), the filterbank
# on each batch of frames, the normaliser behind it; offline, the same three steps one after the other
offline = Pcen.apply(c, Mel.apply(mc, Stft.power_spectrum(sc, clips, power=1.0)))
frames_of = Stft.power_stage(sc, 1.0).prepare(4096)
k = Pcen.Kernel.prepare(c, 2, n_mels)
spectra = [frames_of.step(clips[:, a:a + 4096]) for a in range(0, clips.shape[-1], 4096)] + frames_of.flush()
parts = [k.step(Mel.apply(mc, s)) for s in spectra if s is not None and s.shape[-1] > 0] + k.flush()
streamed = np.concatenate(parts, axis=-1)
print("streamed in chunks of 4096 samples: %d frames, equal to the offline steps bit for bit: %s" % (streamed.shape[-1], np.array_equal(streamed, offline)))
print("the fused call against the three steps: %.3g relative at most" % float(np.max(np.abs(P.cpu().numpy() - offline) / np.maximum(offline, 1e-30))))
