"""Listen to a mel spectrogram and to an MFCC matrix: analyse a batch of resident clips, throw the waveform away, and come back
through Mel.invert (a non-negative least-squares solve per frame) and Griffin-Lim, without anything leaving the device.

    python examples/mel_to_audio.py
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import soundml_amd as S  # noqa: E402
from soundml_amd import Convert, Mel, Stft  # noqa: E402

rate, seconds, fft, hop, n_mels = 22050, 3, 2048, 512, 128
t = np.arange(rate * seconds) / rate
clips = np.stack([0.4 * np.sin(2 * np.pi * f * t) + 0.2 * np.sin(2 * np.pi * 3 * f * t) for f in (220.0, 330.0, 523.25)])
x = torch.from_numpy(clips.astype(np.float32)).cuda()              # [3; n], resident

sc = Stft.Config.create(fft_size=fft, hop=hop)
mc = Mel.Config.create(n_mels=n_mels, sample_rate=rate, fft_size=fft)
mel = S.mel_spectrogram(sc, mc, x)                                 # [3; 128; frames], powers

power = Mel.invert(mc, mel)                                        # [3; 1025; frames] >= 0, 200 rounds per frame in one launch
back = Mel.apply(mc, power)
print("Mel.invert: |W s - m| / |m| = %.2e over the batch" % float((back - mel).norm() / mel.norm()))
truth = Stft.power_spectrum(sc, x)
print("            against the spectrogram the mels came from: %.1f %% of its energy apart (the mel bank forgets that much)"
      % (100.0 * float((power - truth).norm() / truth.norm())))

y = S.mel_to_audio(sc, mc, mel, length=x.shape[-1])                # mel_to_stft (the square root of the solve) + Griffin-Lim
again = S.mel_spectrogram(sc, mc, y)
print("mel_to_audio: %s on %s; the mel spectrogram of the result is %.1f dB under the original's in error"
      % (tuple(y.shape), y.device, -10.0 * np.log10(float(((again - mel) ** 2).sum() / (mel ** 2).sum()))))

c = S.mfcc(sc, mc, x, n_mfcc=20)                                   # [3; 20; frames]
smooth = S.mfcc_to_mel(c, n_mels)                                  # 20 of 128 cepstral rows: the envelope of the log-mels
db = Convert.power_to_db(mel, top_db=80.0)
print("mfcc_to_mel from 20 coefficients: %.1f dB rms apart from the clamped log-mel spectrogram"
      % float((Convert.power_to_db(smooth) - db).square().mean().sqrt()))
z = S.mfcc_to_audio(sc, mc, c, length=x.shape[-1])
print("mfcc_to_audio: %s; peak %.2f (the originals': %.2f)" % (tuple(z.shape), float(z.abs().max()), float(x.abs().max())))
print("a MIDI note for each clip's fundamental: %s" % np.round(Convert.hz_to_midi(np.array([220.0, 330.0, 523.25])), 2).tolist())
