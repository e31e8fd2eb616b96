"""A constant-Q chromagram of a C major arpeggio: the octave recursion, the filter banks and the fold all run on the device.

    python examples/chroma_cqt.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from soundml_amd import Chroma, Cqt, chroma_cqt  # noqa: E402

rate, note_seconds = 22050, 0.5
notes = [("C4", 261.6255653005986), ("E4", 329.6275569128699), ("G4", 391.99543598174927), ("C5", 523.2511306011972)]
t = np.arange(int(rate * note_seconds)) / rate
x = np.concatenate([0.5 * np.sin(2 * np.pi * f * t) * np.hanning(t.size) for _, f in notes]).astype(np.float32)

c = Cqt.Config.create(n_bins=84, sample_rate=rate)            # C1 upward, 12 bins per octave, hop 512
print(c)
print("octaves (first bin, bins, n_fft, hop, halvings):", c.octaves)
magnitudes = Cqt.power_spectrum(c, x, power=1.0)               # [84; frames]
chroma = chroma_cqt(c, x)                                      # [12; frames], each frame scaled to a maximum of 1
names = ["C", "C#", "D", "D#", "E", "F", "F#", "G", "G#", "A", "A#", "B"]
frequencies = Cqt.frequencies(np.float64, c)
for i, (name, f) in enumerate(notes):
    frame = int((i + 0.5) * t.size / c.hop)
    print("%s (%.1f Hz): loudest bin at %.1f Hz, pitch class %s" % (name, f, frequencies[int(np.argmax(magnitudes[:, frame]))],
                                                                    names[int(np.argmax(chroma[:, frame]))]))

# the same chromagram of a live signal: Chroma.of_cqt on the magnitudes a streaming kernel emits, chunk by chunk.  A column leaves
# `latency` samples after its centre went in; the flush returns the rest.  The columns are the offline ones, bit for bit.
kernel = Cqt.Kernel.prepare(c, channels=1, max_block=4096, power=1.0)
print("streaming: latency %d samples, at most %d columns per step" % (kernel.latency, kernel.column_bound))
pieces = [kernel.step(x[None, lo:lo + 4096]) for lo in range(0, x.size, 4096)] + [kernel.flush()]
live = np.concatenate([Chroma.of_cqt(c, m) for m in pieces if m is not None], axis=-1)[0]
print("columns per step:", [0 if m is None else m.shape[-1] for m in pieces], "equal to the offline chromagram:", np.array_equal(live, chroma))
