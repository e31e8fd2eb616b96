"""Device time of Effects on the C2 shapes (256 clips of 480000 samples; 256 x 1025 x 938 complex64 spectra): HIP events
around one call, device-resident in and out, median of --steps after --warmup.  One case per process, so that a launcher can
give each its own time limit:

    for c in vocoder_independent_0.8 vocoder_independent_1.25 vocoder_locked_0.8 vocoder_locked_1.25 \
             time_stretch_0.8 time_stretch_1.25 time_stretch_locked_0.8 pitch_shift round_trip cpu; do
        timeout -k 10 300 python tools/bench_effects.py --case $c || break
    done

    vocoder_<phase>_<rate>     phase_vocoder on complex64 [clips; 1025; 938]
    time_stretch[_locked]_<rate>  time_stretch from audio [clips; 480000] (transform + vocoder + invert, chunked)
    pitch_shift                pitch_shift at semitones(4) = 349/277 (time_stretch at 277/349, resample 349 -> 277, cut)
    round_trip                 Stft.transform + Stft.invert alone on the same audio
    cpu                        the numpy restatement (tests/effects_restatement.py) of the vocoder on ONE clip, on the host

Each line is JSON: median / min milliseconds, cells, the 16 B per cell copy floor (8 read, 8 written, the written side scaled
by 1 / rate) and its fraction of the 6.29 TB/s measured-copy roof."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ROOF = 6.29e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", required=True)
    ap.add_argument("--clips", type=int, default=256)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    bins, frames, n = 1025, 938, 480000
    import numpy as np

    if a.case == "cpu":
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import effects_restatement as R
        rng = np.random.default_rng(0)
        z = (rng.standard_normal((bins, frames)) + 1j * rng.standard_normal((bins, frames))).astype(np.complex64)
        for locked in (False, True):
            t0 = time.perf_counter()
            R.vocode(2048, 512, z, 0.8, locked=locked)
            ms = (time.perf_counter() - t0) * 1e3
            print(json.dumps({"case": "cpu restatement (numpy, one clip, host), %s, rate 0.8" % ("locked" if locked else "independent"),
                              "clips": 1, "cells": bins * frames, "ms": round(ms, 1)}))
        return

    import torch
    import soundml_amd as S  # noqa: F401
    from soundml_amd import Effects, Stft

    torch.manual_seed(0)
    clips = a.clips
    cells = clips * bins * frames
    c = Stft.Config.create(fft_size=2048, hop=512)
    parts = a.case.split("_")
    if parts[0] == "vocoder":
        phase, rate = parts[1], float(parts[2])
        z = torch.view_as_complex(torch.randn(clips, bins, frames, 2, device="cuda:0"))
        run, nbytes = (lambda: Effects.phase_vocoder(c, z, rate, phase=phase)), cells * (8 + 8 / rate)
    elif a.case.startswith("time_stretch"):
        phase, rate = ("locked" if "locked" in parts else "independent"), float(parts[-1])
        x = torch.rand(clips, n, device="cuda:0") * 2 - 1
        run, nbytes = (lambda: Effects.time_stretch(c, x, rate, phase=phase)), cells * (8 + 8 / rate)
    elif a.case == "pitch_shift":
        ratio = Effects.semitones(4)
        x = torch.rand(clips, n, device="cuda:0") * 2 - 1
        run, nbytes = (lambda: Effects.pitch_shift(c, x, ratio)), cells * (8 + 8 * ratio[0] / ratio[1])
    elif a.case == "round_trip":
        x = torch.rand(clips, n, device="cuda:0") * 2 - 1
        run, nbytes = (lambda: Stft.invert(c, Stft.transform(c, x), length=n)), cells * 16
    else:
        raise SystemExit("unknown case %s" % a.case)
    for _ in range(a.warmup):
        run()
    torch.cuda.synchronize()
    times = []
    for _ in range(a.steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    times.sort()
    med = times[len(times) // 2]
    print(json.dumps({"case": a.case, "clips": clips, "cells": cells, "steps": a.steps, "ms_median": round(med, 3), "ms_min": round(times[0], 3),
                      "ns_per_cell": round(med * 1e6 / cells, 4), "copy_floor_bytes": int(nbytes),
                      "copy_floor_ms": round(nbytes / ROOF * 1e3, 3), "fraction_of_copy_roof": round(nbytes / (med * 1e-3) / ROOF, 4)}))


if __name__ == "__main__":
    main()
