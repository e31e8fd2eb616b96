"""Device time of Pcen on a resident float32 mel spectrogram [clips; bands; frames]: HIP events around --inner calls in a row, the
median over --steps such windows after --warmup, per call.  The cases of one shape run interleaved in one process (a round times
each case once), so a clock or thermal drift meets them all alike.  One shape per process, so that a launcher can give each its own
time limit:

    for s in 256x128x431 256x128x938 256x80x3000; do
        timeout -k 10 300 python tools/bench_pcen.py --shape $s --out profiles/pcen/bench_pcen.jsonl || break
    done

    apply            Pcen.apply (the tile kernel)
    smooth           Pcen.smooth (the same kernel without the compression)
    general          Pcen.apply with SMX_DISABLE_FAST=1 (a lane per row)
    composition      what the library offered before: Iir.apply with the one-pole section [[s, 0, 0, 1, s - 1, 0]] over the scaled
                     spectrogram from lfilter_zi's start, then the same expressions in torch float64 on the device
    pcen_from_audio / mel_spectrogram   pcen(...) of the audio that gives this many frames at fft 2048 / hop 512, next to
                     mel_spectrogram alone (bands must be a mel count)
    kernel_step      one Pcen.Kernel step of 8 frames x clips x bands in mid-stream

--out replaces the lines of this shape in the file (a second run leaves no duplicates) and keeps those of other shapes; every line
carries the UTC time of its run and the frames it timed (`kernel_step` times 8 frames whatever the shape's name says).  Before
anything is timed, `apply` must agree with the composition within 1e-6 relative: the composition rounds the smoother to float32
once more than `apply` does, a few float32 ulps through the gain, and nothing else separates them.

Each line is JSON: median / min / max milliseconds per call and the yardsticks: one read plus one write of the tensor at the 8 TB/s of
the data sheet, and the compression's 273 float64 instructions per cell at the 3.66e13 per second this project measured."""
import argparse
import contextlib
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK_BYTES_PER_S = 8e12
F64_PER_CELL, F64_PER_S = 273, 3.66e13


@contextlib.contextmanager
def general_route():
    os.environ["SMX_DISABLE_FAST"] = "1"
    try:
        yield
    finally:
        os.environ.pop("SMX_DISABLE_FAST", None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="256x128x938")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    clips, bands, frames = (int(v) for v in a.shape.split("x"))

    import torch
    import soundml_amd as S
    from soundml_amd import Iir, Mel, Pcen, Stft

    torch.manual_seed(0)
    scale = 2.0 ** 31
    c = Pcen.Config.create(scale=scale)
    x = torch.rand(clips, bands, frames, device="cuda:0") ** 8 * 1e-3
    s = c.coefficient
    ci = Iir.Config.create([[s, 0.0, 0.0, 1.0, s - 1.0, 0.0]])
    log_eps, bias_pow = math.log(c.eps), c.bias ** c.power

    def composition():
        u = x * scale
        zi = torch.stack([(1.0 - s) * u[..., 0].double(), torch.zeros_like(u[..., 0], dtype=torch.float64)], -1).unsqueeze(-2)
        M = Iir.apply(ci, u, zi=zi).double()
        sm = torch.exp(-c.gain * (log_eps + torch.log1p(M / c.eps)))
        return (bias_pow * torch.expm1(c.power * torch.log1p(u.double() * sm / c.bias))).float()

    def general():
        with general_route():
            return Pcen.apply(c, x)

    hop = 512
    sc, mc = Stft.Config.create(fft_size=2048, hop=hop), Mel.Config.create(n_mels=bands, sample_rate=22050, fft_size=2048)
    audio = torch.rand(clips, (frames - 1) * hop, device="cuda:0") * 2 - 1
    assert Stft.frames(sc, audio.shape[-1]) == frames
    k = Pcen.Kernel.prepare(c, clips, bands)
    chunk = x[..., :8].contiguous()
    k.step(chunk)
    cases = {
        "apply": lambda: Pcen.apply(c, x),
        "smooth": lambda: Pcen.smooth(c, x),
        "general": general,
        "composition": composition,
        "pcen_from_audio": lambda: S.pcen(sc, mc, audio, c),
        "mel_spectrogram": lambda: S.mel_spectrogram(sc, mc, audio, power=1.0),
        "kernel_step": lambda: k.step(chunk),
    }
    got, want = Pcen.apply(c, x), composition()
    apart = float(((got - want).abs() / want.abs().clamp_min(1e-30)).max())
    print("apply against the composition: %.3g relative at most" % apart, file=sys.stderr)
    assert apart <= 1e-6, "apply and the composition it is timed against do not compute the same thing"
    del got, want
    stamp = time.strftime("%Y-%m-%dT%H:%M:%SZ", time.gmtime())
    for _ in range(a.warmup):
        for run in cases.values():
            run()
    torch.cuda.synchronize()
    times = {name: [] for name in cases}
    for _ in range(a.steps):
        for name, run in cases.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.inner):
                run()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / a.inner)
    lines = []
    for name, t in times.items():
        t.sort()
        timed = 8 if name == "kernel_step" else frames
        cells = clips * bands * timed
        roof = 2 * 4 * cells / PEAK_BYTES_PER_S * 1e3
        f64 = cells * F64_PER_CELL / F64_PER_S * 1e3
        med = t[len(t) // 2]
        lines.append({"case": name, "shape": a.shape, "frames_timed": timed, "run": stamp, "apply_vs_composition_rel": apart, "steps": a.steps, "inner": a.inner, "ms_median": round(med, 4), "ms_min": round(t[0], 4),
                      "ms_max": round(t[-1], 4), "cells": cells, "ms_read_write_at_8TBs": round(roof, 4), "multiple_of_roof": round(med / roof, 2),
                      "ms_f64_at_3.66e13": round(f64, 4), "multiple_of_f64": round(med / f64, 2)})
    by = {l["case"]: l["ms_median"] for l in lines}
    for l in lines:
        l["apply_over_this"] = round(by["apply"] / l["ms_median"], 3)
        print(json.dumps(l))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        kept = []
        if os.path.exists(a.out):
            with open(a.out) as fh:
                kept = [r for r in fh if r.strip() and json.loads(r).get("shape") != a.shape]
        with open(a.out, "w") as fh:
            fh.writelines(kept)
            for l in lines:
                fh.write(json.dumps(l) + "\n")


if __name__ == "__main__":
    main()
