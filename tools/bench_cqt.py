"""Device time of Cqt.power_spectrum and chroma_cqt on 256 clips of 10 s, next to the baseline a user had before: the same
plan composed from public calls (Resample.apply for the 2:1 stages, Stft.transform with a rectangular window under the float64
interior (the float32 one at sizes where the public transform has no float64 form), one torch complex matmul with the half-spectrum matrix K per octave).  HIP events around one call, device-resident in
and out, median of --steps after --warmup.  One (plan, rate) per process, so that a launcher can give each its own limit:

    for rate in 22050 48000; do for plan in c1_hop512 c1_hop511 bpo36; do
        timeout -k 10 300 python tools/bench_cqt.py --plan $plan --rate $rate || break
    done; done
    timeout -k 10 300 python tools/bench_cqt.py --plan c1_hop512 --rate 22050 --profile traces/cqt   # per-kernel times

    c1_hop512   84 bins from C1, 12 per octave, hop 512 (seven octaves, six 2:1 stages between them)
    c1_hop511   the same ladder at hop 511: no decimation, every octave at the input rate, n_fft 256 .. 16384 (22050 Hz)
    bpo36       252 bins from C1, 36 per octave, hop 512

Each line is JSON.  ``power`` / ``chroma``: the library call.  ``chain``: the plan's Resample.apply calls alone (the share of
the library call that is decimation).  ``baseline``: the composition, in clip chunks of --baseline-chunk (its per-octave
complex spectra do not fit otherwise), times summed.  ``flops`` counts 4 n_fft flops per (bin, frame) of the projection.
--profile DIR runs ``rocprofv3 --kernel-trace --stats`` over a child process (three steps of ``power``) and prints the
kernels' total and average times from its statistics.

--stream CHUNK times the streaming ``Cqt.Kernel`` instead: the same clips fed in chunks of CHUNK samples, HIP events around
every ``step``.  ``stream``: the median and least time of a steady-state step (every octave is producing: the gate has opened),
the total of all steps and the flush, and the library's kernel launches per steady-state step, its own three (append, project,
emit) apart from the 2:1 stages'.  ``rerun``: what a user had before -- ``Cqt.transform`` of the last latency + CHUNK samples, for
every chunk.  ``offline``: one ``Cqt.transform`` of the whole signal, next to the stream's total.  With --profile the child
streams (one pass), and the statistics are per kernel over that pass."""
import argparse
import csv
import glob
import json
import math
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PLANS = {"c1_hop512": dict(n_bins=84, hop=512), "c1_hop511": dict(n_bins=84, hop=511), "bpo36": dict(n_bins=252, bins_per_octave=36, hop=512)}


def timed(torch, run, steps, warmup):
    for _ in range(warmup):
        run()
    torch.cuda.synchronize()
    times = []
    for _ in range(steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    times.sort()
    return times[len(times) // 2], times[0]


def profile(a):
    os.makedirs(a.profile, exist_ok=True)
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", a.profile, "--", sys.executable, os.path.abspath(__file__),
           "--plan", a.plan, "--rate", str(a.rate), "--clips", str(a.clips), "--seconds", str(a.seconds), "--steps", "3", "--warmup", "1",
           "--only", "power"]
    if a.stream:
        cmd += ["--stream", str(a.stream)]
    subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL)
    rows = []
    for path in glob.glob(os.path.join(a.profile, "**", "*kernel_stats.csv"), recursive=True):
        with open(path) as fh:
            rows += list(csv.DictReader(fh))
    total = sum(float(r["TotalDurationNs"]) for r in rows) or 1.0
    for r in sorted(rows, key=lambda r: -float(r["TotalDurationNs"])):
        print(json.dumps({"plan": a.plan, "rate": a.rate, "kernel": r["Name"][:120], "calls": int(r["Calls"]),
                          "total_ms": round(float(r["TotalDurationNs"]) * 1e-6, 3), "average_ms": round(float(r["AverageNs"]) * 1e-6, 4),
                          "share": round(float(r["TotalDurationNs"]) / total, 4)}))


def stream(a, torch, Cqt, c, x, common):
    from soundml_amd._lib import lib
    n, chunk = x.shape[-1], a.stream
    kern = Cqt.Kernel.prepare(c, channels=a.clips, max_block=chunk)
    cuts = list(range(0, n, chunk)) + [n]
    common = dict(common, chunk=chunk, latency=c.latency, chunks=len(cuts) - 1)

    def one_pass():
        kern.reset()
        torch.cuda.synchronize()
        events, launches = [], []
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            e0, e1, l0 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True), lib.smx_debug_kernel_launches()
            e0.record()
            out = kern.step(x[:, lo:hi])
            e1.record()
            events.append((lo, hi, e0, e1))
            launches.append(lib.smx_debug_kernel_launches() - l0)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        kern.flush()
        e1.record()
        torch.cuda.synchronize()
        times = [(lo, hi, e0_.elapsed_time(e1_)) for lo, hi, e0_, e1_ in events]
        return times, e0.elapsed_time(e1), launches

    passes = 1 if a.only == "power" else max(1, a.warmup) + max(1, a.steps // 3)   # --only power: the profiled child
    for k in range(passes):
        times, flush_ms, launches = one_pass()
    full = [lo >= c.latency + chunk and hi - lo == chunk for lo, hi, _ in times]   # the gate is open, and the chunk is whole
    steady = sorted(t for (_, _, t), ok in zip(times, full) if ok)
    steady_launches = [l for l, ok in zip(launches, full) if ok]
    line = dict(common, case="stream", steady_steps=len(steady), flush_ms=round(flush_ms, 3),
                total_ms=round(sum(t for _, _, t in times) + flush_ms, 3), decimator_stages=common["decimations"],
                launches_per_steady_step=max(steady_launches) if steady_launches else None)
    if steady:
        line.update(ms_median=round(steady[len(steady) // 2], 4), ms_min=round(steady[0], 4))
    print(json.dumps(line), flush=True)
    if a.only == "power":
        return
    window = min(n, c.latency + chunk)
    tail = x[:, n - window:]
    med, least = timed(torch, lambda: Cqt.transform(c, tail), a.steps, a.warmup)
    print(json.dumps(dict(common, case="rerun", window=window, ms_median=round(med, 4), ms_min=round(least, 4))), flush=True)
    med, least = timed(torch, lambda: Cqt.transform(c, x), max(3, a.steps // 3), 1)
    print(json.dumps(dict(common, case="offline", ms_median=round(med, 3), ms_min=round(least, 3))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--plan", required=True, choices=sorted(PLANS))
    ap.add_argument("--rate", type=int, default=22050)
    ap.add_argument("--clips", type=int, default=256)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--baseline-chunk", type=int, default=32)
    ap.add_argument("--only", default="")
    ap.add_argument("--profile", default="")
    ap.add_argument("--stream", type=int, default=0, metavar="CHUNK")
    a = ap.parse_args()
    if a.profile:
        return profile(a)

    import numpy as np
    import torch
    import soundml_amd as S
    from soundml_amd import Cqt, Resample, Stft

    n = int(a.rate * a.seconds)
    c = Cqt.Config.create(sample_rate=a.rate, **PLANS[a.plan])
    half = Resample.Config.create(2, 1, "high")
    count = Cqt.frames(c, n)
    octaves = c.octaves
    flops = 4.0 * a.clips * count * sum(cnt * n_fft for _, cnt, n_fft, _, _ in octaves)
    stages = c.early + sum(1 for i, o in enumerate(octaves[:-1]) if o[3] % 2 == 0)
    torch.manual_seed(0)
    x = torch.rand(a.clips, n, device="cuda:0") * 2 - 1
    common = {"plan": a.plan, "rate": a.rate, "clips": a.clips, "samples": n, "frames": count, "bins": c.n_bins, "early": c.early,
              "octaves": [list(o) for o in octaves], "decimations": stages, "steps": a.steps}

    def report(case, med, least, **more):
        print(json.dumps(dict(common, case=case, ms_median=round(med, 3), ms_min=round(least, 3), **more)), flush=True)

    if a.stream:
        return stream(a, torch, Cqt, c, x, common)

    def chain():
        y = x
        for _ in range(stages):
            y = Resample.apply(half, y)
        return y

    # the composition: K per octave from the library's own taps (K is the first n_fft / 2 + 1 entries of their inverse transform)
    kernels = [torch.from_numpy(np.fft.ifft(c.taps(i), axis=1)[:, :o[2] // 2 + 1].astype(np.complex64)).to("cuda:0") for i, o in enumerate(octaves)]
    configs = [Stft.Config.create(fft_size=o[2], window="rectangular", hop=o[3], pad=("constant", 0.0)) for o in octaves]
    divisors = torch.from_numpy(c.divisors().astype(np.float32)).to("cuda:0")[:, None]
    unavailable = None
    interiors = []   # the float64 interior where the public transform has it at this size, else the float32 one
    for cfg in (configs if a.only in ("", "baseline") else []):
        S.set_interior("float64")
        try:
            Stft.transform(cfg, x[:1])
            interiors.append("float64")
        except S.Failure:
            S.set_interior("float32")
            try:
                Stft.transform(cfg, x[:1])
                interiors.append("float32")
            except S.Failure as e:   # no public transform at this size: the composition does not exist for this plan
                interiors.append(None)
                unavailable = str(e)
        S.set_interior("float32")
    common["baseline_interiors"] = interiors

    def baseline_chunk(xc):
        y = xc
        for _ in range(c.early):
            y = Resample.apply(half, y)
        if c.early:
            y = y * math.sqrt(float(1 << c.early))
        out = torch.empty((xc.shape[0], c.n_bins, count), dtype=torch.complex64, device=xc.device)
        for i, (first, cnt, _, hop, _) in enumerate(octaves):
            S.set_interior(interiors[i])
            d = Stft.transform(configs[i], y)[..., :count]
            out[:, first:first + cnt] = torch.matmul(kernels[i], d)
            if i < len(octaves) - 1 and hop % 2 == 0:
                y = Resample.apply(half, y) / math.sqrt(0.5)
        return (out / divisors).abs()

    def baseline():
        try:
            return [baseline_chunk(x[k:k + a.baseline_chunk]) for k in range(0, a.clips, a.baseline_chunk)]
        finally:
            S.set_interior("float32")

    cases = {"power": lambda: Cqt.power_spectrum(c, x, power=1.0), "chroma": lambda: S.chroma_cqt(c, x), "chain": chain, "baseline": baseline}
    for case, run in cases.items():
        if a.only and case != a.only:
            continue
        if case == "baseline" and unavailable:
            print(json.dumps(dict(common, case=case, unavailable=unavailable)), flush=True)
            continue
        med, least = timed(torch, run, a.steps if case != "baseline" else max(3, a.steps // 3), a.warmup if case != "baseline" else 1)
        more = {"projection_flops": flops, "tflops_of_whole_call": round(flops / (med * 1e-3) / 1e12, 3)} if case == "power" else {}
        report(case, med, least, **more)
    if not a.only and not unavailable:   # the two must agree before their times are compared
        got = Cqt.power_spectrum(c, x[:2], power=1.0)
        want = baseline_chunk(x[:2])
        S.set_interior("float32")
        peak = float(want.abs().max())
        print(json.dumps(dict(common, case="agreement", worst_deviation_of_peak=float((got - want).abs().max()) / peak)), flush=True)


if __name__ == "__main__":
    main()
