"""Device time of Loudness on 128 stereo clips x 480000 samples (256 channels, 10 s at 48 kHz), float32, device-resident in and
out: HIP events around --inner calls in a row, the median over --steps such windows after --warmup, per call.  One case per
process, so that a launcher can give each its own time limit:

    for c in integrated block_energy true_peak normalize normalize_ceiling meter_step composition resample_peak; do
        timeout -k 10 300 python tools/bench_loudness.py --case $c || break
    done

    integrated / block_energy / true_peak / normalize / normalize_ceiling   the faces on the resident audio
    meter_step       one Loudness.Meter step of 4096 samples x 256 channels in mid-stream
    composition      what the library offered before: Iir.apply with the same sections, then unfold, square and mean in torch
    resample_peak    the yardstick of true_peak: Resample.apply(4 / 1, "high") of the audio, then abs and amax in torch

Each line is JSON: median / min / max milliseconds per call, the bytes of one read of the audio and the time they take at the
8 TB/s of the data sheet."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK_BYTES_PER_S = 8e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", required=True)
    ap.add_argument("--clips", type=int, default=128)
    ap.add_argument("--channels", type=int, default=2)
    ap.add_argument("--samples", type=int, default=480000)
    ap.add_argument("--rate", type=int, default=48000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=5)
    a = ap.parse_args()

    import torch
    from soundml_amd import Iir, Loudness, Resample

    torch.manual_seed(0)
    x = (torch.rand(a.clips, a.channels, a.samples, device="cuda:0") * 2 - 1) * 0.1
    step = Loudness.step(a.rate)
    if a.case == "integrated":
        run = lambda: Loudness.integrated(x, a.rate)
    elif a.case == "block_energy":
        run = lambda: Loudness.block_energy(x, a.rate)
    elif a.case == "true_peak":
        run = lambda: Loudness.true_peak(x)
    elif a.case == "normalize":
        run = lambda: Loudness.normalize(x, a.rate)
    elif a.case == "normalize_ceiling":
        run = lambda: Loudness.normalize(x, a.rate, peak_ceiling=10.0 ** (-1.0 / 20.0))
    elif a.case == "meter_step":
        x = x[..., :4096].contiguous()
        k = Loudness.Meter.prepare(a.rate, a.clips, a.channels)
        k.step(x[..., :1000].contiguous())          # mid-stream: the step begins and ends inside an Iir block
        run = lambda: k.step(x)
    elif a.case == "composition":
        c = Iir.Config.create(Loudness.k_weighting(a.rate))
        run = lambda: Iir.apply(c, x).unfold(-1, 4 * step, step).square().mean(-1)
    elif a.case == "resample_peak":
        c = Resample.Config.create(4, 1, "high")
        run = lambda: Resample.apply(c, x).abs().amax(-1)
    else:
        raise SystemExit("unknown case %s" % a.case)
    nbytes = x.numel() * 4
    for _ in range(a.warmup):
        run()
    torch.cuda.synchronize()
    times = []
    for _ in range(a.steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.inner):
            run()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) / a.inner)
    times.sort()
    roof = nbytes / PEAK_BYTES_PER_S * 1e3
    line = {"case": a.case, "clips": a.clips, "channels": a.channels, "samples": int(x.shape[-1]), "rate": a.rate, "steps": a.steps, "inner": a.inner,
            "ms_median": round(times[len(times) // 2], 4), "ms_min": round(times[0], 4), "ms_max": round(times[-1], 4), "read_bytes": nbytes,
            "ms_read_at_8TBs": round(roof, 4), "multiple_of_roof": round(times[len(times) // 2] / roof, 2)}
    print(json.dumps(line))


if __name__ == "__main__":
    main()
