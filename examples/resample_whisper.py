#!/usr/bin/env python3
"""44.1 kHz clips -> 16 kHz -> whisper's log-mel front end (fft 400 / hop 160, 80 mel bands, log10 clamped 8 dB under the
loudest cell, (v + 4) / 4), all on the device: `soundml_amd.resample` designs the 160/441 conversion (K = 261, `High
quality) and runs it on the polyphase kernel; the fused mel spectrogram takes the result where it lies.
Needs a HIP device (there is no CPU fallback)."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from soundml_amd import Mel, Resample, Stft, mel_spectrogram, resample   # noqa: E402

sr, target, seconds, clips = 44100, 16000, 30, 8
t = torch.arange(sr * seconds, device="cuda", dtype=torch.float64) / sr
tones = torch.tensor([220.0 * 2 ** (i / 4) for i in range(clips)], device="cuda", dtype=torch.float64)
x = torch.sin(2 * torch.pi * tones[:, None] * t[None, :]).float()       # [8; 1 323 000] at 44.1 kHz, device-resident

cfg = Resample.Config.create(sr, target)
print(cfg, "-- latency", cfg.latency, "input samples")
y = resample(x, sr, target)                                              # = Resample.apply(cfg, x): [8; 480 000] at 16 kHz
stft = Stft.Config.create(fft_size=400, hop=160)
mel = Mel.Config.create(n_mels=80, sample_rate=target, fft_size=400)
m = mel_spectrogram(stft, mel, y)[..., :-1]                              # whisper drops the last frame: [8; 80; 3000]
log = torch.clamp(m, min=1e-10).log10()
log = torch.maximum(log, log.amax(dim=(-2, -1), keepdim=True) - 8.0)
feat = (log + 4.0) / 4.0
torch.cuda.synchronize()
print("audio", tuple(x.shape), "->", tuple(y.shape), "-> log-mel", tuple(feat.shape), "on", feat.device)
print("loudest mel band per clip:", feat.mean(dim=-1).argmax(dim=-1).tolist())
