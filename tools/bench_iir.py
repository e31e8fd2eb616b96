"""Device time of Iir on 256 channels x 480000 samples (10 s at 48 kHz), float32, device-resident in and out: HIP events around
--inner calls in a row, the median over --steps such windows after --warmup, per call.  One case per process, so that a launcher
can give each its own time limit:

    for s in 1 2 4 8; do for c in apply apply_general; do
        timeout -k 10 300 python tools/bench_iir.py --case $c --sections $s || break 2
    done; done

    apply            Iir.apply on the resident audio: the block route (two block passes and the state chain between them)
    apply_general    the same with SMX_DISABLE_FAST: a lane per channel walks the samples (give it --steps 3 --inner 1 --warmup 1)
    filtfilt         Iir.filtfilt: two passes over the extended signal, the float64 intermediate in scratch
    kernel_step      one Iir.Kernel step of 4096 samples x 256 channels in mid-stream

The sections are the first --sections of the test cascade (tests/iir_restatement.py: a Butterworth low-pass, a 20 Hz high-pass and
the two K-weighting biquads in turn); the time does not depend on the coefficients.  Each line is JSON: median / min / max
milliseconds per call, the bytes of one read plus one write of the audio and the time they take at the 8 TB/s of the data sheet."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
PEAK_BYTES_PER_S = 8e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", required=True)
    ap.add_argument("--sections", type=int, default=4)
    ap.add_argument("--clips", type=int, default=256)
    ap.add_argument("--samples", type=int, default=480000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=5)
    a = ap.parse_args()

    import torch
    from soundml_amd import Iir
    import iir_restatement as R

    torch.manual_seed(0)
    c = Iir.Config.create(R.cascade(a.sections))
    x = torch.rand(a.clips, a.samples, device="cuda:0") * 2 - 1
    if a.case == "apply_general":
        os.environ["SMX_DISABLE_FAST"] = "1"
    if a.case in ("apply", "apply_general"):
        run = lambda: Iir.apply(c, x)
    elif a.case == "filtfilt":
        run = lambda: Iir.filtfilt(c, x)
    elif a.case == "kernel_step":
        x = x[:, :4096].contiguous()
        k = Iir.Kernel.prepare(c, a.clips)
        k.step(x[:, :1000].contiguous())            # mid-stream: the step begins and ends inside a block
        run = lambda: k.step(x)
    else:
        raise SystemExit("unknown case %s" % a.case)
    nbytes = 2 * x.numel() * 4
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
    line = {"case": a.case, "sections": a.sections, "clips": a.clips, "samples": int(x.shape[-1]), "block": Iir.BLOCK, "steps": a.steps,
            "inner": a.inner, "ms_median": round(times[len(times) // 2], 4), "ms_min": round(times[0], 4), "ms_max": round(times[-1], 4),
            "read_plus_write_bytes": nbytes, "ms_read_plus_write_at_8TBs": round(roof, 4), "multiple_of_roof": round(times[len(times) // 2] / roof, 2)}
    print(json.dumps(line))


if __name__ == "__main__":
    main()
