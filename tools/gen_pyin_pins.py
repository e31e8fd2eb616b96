"""Pins of pYIN's host tables from scipy, written once on the CPU into tests/golden/pitch/pyin_pins.json; the tests read only the JSON.

    python tools/gen_pyin_pins.py

  beta        scipy.stats.beta.cdf differences over thr[k] = k / n for (a, b) in (2, 18), (1, 1), (0.5, 3.5) at n = 100 and n = 7
  boltzmann   scipy.stats.boltzmann.pmf(q, lambda, N) for q < N: the ONE product Z[N] * E[q] of the definition
  bins        n_bins = floor(12 bps log2(fmax / fmin)) + 1 and h = (round-half-even(rate 12 hop / sr) bps) // 2 for a few geometries"""
import json
import math
import os

import numpy as np
from scipy import stats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    pins = {"beta": [], "boltzmann": [], "bins": [], "half_width": []}
    for a, b in ((2.0, 18.0), (1.0, 1.0), (0.5, 3.5)):
        for n in (100, 7):
            cdf = stats.beta.cdf(np.arange(n + 1) / float(n), a, b)
            pins["beta"].append({"a": a, "b": b, "n": n, "values": np.diff(cdf).tolist()})
    for lam in (2.0, 0.5):
        for N in (1, 2, 5, 40):
            pins["boltzmann"].append({"lambda": lam, "N": N, "values": stats.boltzmann.pmf(np.arange(N), lam, N).tolist()})
    for fmin, fmax, resolution in ((65.0, 2093.0, 0.1), (100.0, 1000.0, 0.1), (400.0, 500.0, 0.1), (100.0, 1000.0, 0.5), (55.0, 880.0, 0.3)):
        bps = math.ceil(1.0 / resolution)
        pins["bins"].append({"fmin": fmin, "fmax": fmax, "resolution": resolution, "n_bins": int(math.floor(12 * bps * math.log2(fmax / fmin))) + 1})
    for sr, hop, resolution, rate in ((22050, 512, 0.1, 35.92), (8000, 64, 0.1, 35.92), (8000, 64, 0.5, 1.0), (22050, 256, 0.3, 35.92), (16000, 160, 0.1, 0.0)):
        bps = math.ceil(1.0 / resolution)
        pins["half_width"].append({"sample_rate": sr, "hop": hop, "resolution": resolution, "max_transition_rate": rate,
                                   "h": (round(rate * 12.0 * hop / sr) * bps) // 2})
    path = os.path.join(ROOT, "tests", "golden", "pitch", "pyin_pins.json")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as fh:
        json.dump(pins, fh, indent=1)
        fh.write("\n")
    print("wrote %s" % path)


if __name__ == "__main__":
    main()
