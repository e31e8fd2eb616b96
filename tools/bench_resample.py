"""Device time of Resample.apply / Resample.Kernel.step of a Resample.Config: HIP events around one call, device-resident in and
out, median of --steps after --warmup.  One case per process, so that a launcher can give each its own time limit (no retries):

    for c in apply_44100_48000 apply_48000_44100 apply_44100_16000 apply_48000_16000 stage_48000_16000 step_44100_48000 step_44100_16000; do
        timeout -k 10 180 python tools/bench_resample.py --case $c >> profiles/resample/bench_resample.jsonl || break
    done

    apply_<sr>_<target>   Resample.apply on --clips clips of --seconds seconds at <sr> Hz
    stage_48000_16000     Resample.Stage.apply on the single-stage /3 design built by hand: what the parent commit can also run
                          (apply_48000_16000 is the same stage reached through Resample.Config)
    step_<sr>_<target>    one Resample.Kernel.step of --block samples x --clips channels in mid-stream

Each line is JSON: median / min milliseconds; the bytes read plus written and their fraction of the 6.29 TB/s measured-copy
roof; for the direct executor the multiply-adds (2 K + 1 per output) and their fraction of the 157.3 TFLOP/s vector FP32 peak
(256 CUs x 128 FMA/clk x 2.4 GHz x 2)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ROOF = 6.29e12
FMA_PEAK = 256 * 128 * 2.4e9    # multiply-adds per second


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", required=True)
    ap.add_argument("--clips", type=int, default=256)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--block", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    kind, sr, target = a.case.split("_")
    sr, target = int(sr), int(target)

    import torch
    from soundml_amd import Resample

    torch.manual_seed(0)
    n = int(round(sr * a.seconds)) if kind != "step" else a.block
    x = torch.rand(a.clips, n, device="cuda:0") * 2 - 1
    row = {"case": a.case, "clips": a.clips, "n": n}
    if kind == "stage":       # the hand-built stage of the parent commit's interface
        from oracle import resample_metrics as M
        import math
        g = math.gcd(sr, target)
        l, m = target // g, sr // g
        k, fc, beta = M.single_stage(l, m)
        st = Resample.Stage.create(Resample.prototype(l, k, fc, beta), l, m, k)
        run = lambda: Resample.Stage.apply(st, x)
        n_out, executor = st.out_length(n), "stage"
    else:
        cfg = Resample.Config.create(sr, target)
        (l, m), k, executor = cfg.rate, cfg.latency, cfg.executor
        n_out = cfg.output_frames(n)
        if kind == "apply":
            run = lambda: Resample.apply(cfg, x)
        elif kind == "step":
            kern = Resample.Kernel.prepare(cfg, a.clips, a.block)
            run = lambda: kern.step(x)
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
    nbytes = 4 * a.clips * (n + n_out)
    row.update({"executor": executor, "l": l, "m": m, "k": k, "n_out": n_out, "steps": a.steps, "ms_median": round(med, 3),
                "ms_min": round(times[0], 3), "bytes": nbytes, "fraction_of_copy_roof": round(nbytes / (med * 1e-3) / ROOF, 4)})
    if executor == "direct":
        fma = a.clips * n_out * (2 * k + 1)
        row.update({"multiply_adds": fma, "fraction_of_fp32_vector_peak": round(fma / (med * 1e-3) / FMA_PEAK, 4)})
    print(json.dumps(row))


if __name__ == "__main__":
    main()
