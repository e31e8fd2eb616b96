"""Writes tests/golden/iir/pins.npz and cases.json: scipy.signal's float64 results for the pinned filters of
tests/test_iir_restatement.py.  Needs scipy (the tests do not); run from the repository root:

    python tools/gen_iir_pins.py

One float32 signal of 6000 samples (seeded).  Per filter: sos, sosfilt of the whole signal, sosfilt_zi, and sosfiltfilt of its
first 2000 samples.  scipy gets the samples widened to float64, so the odd extension is taken in float64 as the library takes it.
"""
import json
import os

import numpy as np
import scipy
from scipy import signal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, N_FILTFILT, SEED = 6000, 2000, 20260

# ITU-R BS.1770-4, table 1 and 2: the K-weighting pre-filter and RLB high-pass at 48 kHz
K_WEIGHTING = np.array([[1.53512485958697, -2.69169618940638, 1.19839281085285, 1.0, -1.69065929318241, 0.73248077421585],
                        [1.0, -2.0, 1.0, 1.0, -1.99004745483398, 0.99007225036621]])

FILTERS = [
    ("butter8_lowpass_0.1", "scipy.signal.butter(8, 0.1, output='sos')", lambda: signal.butter(8, 0.1, output="sos")),
    ("butter4_highpass_20hz_48k", "scipy.signal.butter(4, 20, 'highpass', fs=48000, output='sos')",
     lambda: signal.butter(4, 20, "highpass", fs=48000, output="sos")),
    ("butter8_lowpass_100hz_48k", "scipy.signal.butter(8, 100, fs=48000, output='sos')", lambda: signal.butter(8, 100, fs=48000, output="sos")),
    ("ellip6_bandpass_0.2_0.3", "scipy.signal.ellip(3, 1, 60, [0.2, 0.3], 'bandpass', output='sos')",
     lambda: signal.ellip(3, 1, 60, [0.2, 0.3], "bandpass", output="sos")),
    ("k_weighting_48k", "ITU-R BS.1770-4 tables 1 and 2", lambda: K_WEIGHTING),
]


def main():
    x = np.random.default_rng(SEED).uniform(-1, 1, size=N).astype(np.float32)
    wide = x.astype(np.float64)
    arrays, cases = {"x": x}, []
    for name, how, make in FILTERS:
        sos = np.ascontiguousarray(make(), dtype=np.float64)
        assert np.all(sos[:, 3] == 1.0)
        arrays[name + ".sos"] = sos
        arrays[name + ".sosfilt"] = signal.sosfilt(sos, wide)
        arrays[name + ".sosfilt_zi"] = signal.sosfilt_zi(sos)
        arrays[name + ".sosfiltfilt"] = signal.sosfiltfilt(sos, wide[:N_FILTFILT])
        cases.append({"name": name, "design": how, "sections": int(sos.shape[0])})
    out = os.path.join(ROOT, "tests", "golden", "iir")
    os.makedirs(out, exist_ok=True)
    np.savez_compressed(os.path.join(out, "pins.npz"), **arrays)
    with open(os.path.join(out, "cases.json"), "w") as fh:
        json.dump({"scipy": scipy.__version__, "seed": SEED, "n": N, "n_filtfilt": N_FILTFILT, "cases": cases}, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
