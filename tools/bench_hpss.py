"""Device time of Hpss on the C2-shaped plane stack (256 x 1025 x 938 float32): HIP events around one call, device-resident
in and out, median of --steps after --warmup.  One case per process, so that a launcher can give each its own time limit:

    for c in spectrogram_fast spectrogram_general stft signal round_trip cpu; do
        timeout -k 10 300 python tools/bench_hpss.py --case $c || break
    done

    spectrogram_fast     hpss_of_spectrogram 31 x 31 p = 2, the tile kernel
    spectrogram_general  the same call on the general kernel (SMX_DISABLE_FAST), on --general-clips clips
    stft                 hpss_of_stft 31 x 31 p = 2 on complex64
    signal               hpss from audio [clips; 480000] (transform + hpss_of_stft + two inversions, chunked)
    round_trip           Stft.transform + Stft.invert + Stft.invert alone on the same audio
    cpu                  the numpy restatement (tests/hpss_restatement.py) on ONE clip's plane, on the host

Each line is JSON: median / min milliseconds, cells, the algorithmic bytes (12 B per cell for the real face, 24 B for the
complex one) and their fraction of the 6.29 TB/s measured-copy roof."""
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
    ap.add_argument("--general-clips", type=int, default=16)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    bins, frames, n = 1025, 938, 480000
    import numpy as np

    if a.case == "cpu":
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import hpss_restatement as R
        s = np.random.default_rng(0).random((bins, frames), dtype=np.float32)
        t0 = time.perf_counter()
        R.hpss_of_spectrogram(s)
        ms = (time.perf_counter() - t0) * 1e3
        print(json.dumps({"case": "cpu restatement (numpy, one clip, host)", "clips": 1, "cells": bins * frames, "ms": round(ms, 1)}))
        return

    import torch
    import soundml_amd as S
    from soundml_amd import Hpss, Stft

    torch.manual_seed(0)
    clips = a.general_clips if a.case == "spectrogram_general" else a.clips
    cells = clips * bins * frames
    c = Stft.Config.create(fft_size=2048, hop=512)
    if a.case in ("spectrogram_fast", "spectrogram_general"):
        s = torch.rand(clips, bins, frames, device="cuda:0")
        if a.case == "spectrogram_general":
            os.environ["SMX_DISABLE_FAST"] = "1"
        run, nbytes = (lambda: Hpss.hpss_of_spectrogram(s)), 12 * cells
    elif a.case == "stft":
        z = torch.view_as_complex(torch.randn(clips, bins, frames, 2, device="cuda:0"))
        run, nbytes = (lambda: Hpss.hpss_of_stft(z)), 24 * cells
    elif a.case in ("signal", "round_trip"):
        x = torch.rand(clips, n, device="cuda:0") * 2 - 1
        if a.case == "signal":
            run = lambda: Hpss.hpss(c, x)
        else:
            def run():
                z = Stft.transform(c, x)
                return Stft.invert(c, z, length=n), Stft.invert(c, z, length=n)
        nbytes = 12 * clips * n
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
                      "ns_per_cell": round(med * 1e6 / cells, 4), "algorithmic_bytes": nbytes,
                      "fraction_of_copy_roof": round(nbytes / (med * 1e-3) / ROOF, 4)}))


if __name__ == "__main__":
    main()
