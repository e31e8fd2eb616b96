"""Device time of rms, zero_crossing_rate and rms_of_spectrogram on 256 clips x 10 s (frame_length 2048 / hop 512), float32,
device-resident in and out: HIP events around --inner calls in a row, the median over --steps such windows after --warmup, per
call.  One case per process, so that a launcher can give each its own time limit:

    for r in 22050 48000; do for c in rms zcr rms_general zcr_general rms_spectrogram stage_step power compose; do
        timeout -k 10 300 python tools/bench_energy.py --rate $r --case $c || break 2
    done; done

    rms / zcr           the flat functions on the resident audio (the tile kernel)
    rms_general / zcr_general   the same with SMX_DISABLE_FAST: a wave per frame straight from memory
    rms_spectrogram     rms_of_spectrogram on the resident magnitude spectrogram
    stage_step          one rms_stage step of 4096 samples x 256 channels in mid-stream (concatenation, launch, carry copy)
    power               yardstick (a): Stft.power_spectrum (power 1) on the same audio
    compose             yardstick (b): F.pad, .double().unfold(-1, 2048, 512), square, mean, sqrt, cast in torch

Each line is JSON: median / min / max milliseconds per call, the bytes of one read of the input and the time that read takes
at the 8 TB/s of the data sheet: yardstick (c), computed, the roof of a kernel that reads every sample once."""
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
    ap.add_argument("--rate", type=int, default=22050)
    ap.add_argument("--clips", type=int, default=256)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=5)
    a = ap.parse_args()

    import torch
    import torch.nn.functional as F
    import soundml_amd as S
    from soundml_amd import Stft, energy

    torch.manual_seed(0)
    fl, hop, n = 2048, 512, int(a.rate * a.seconds)
    x = torch.rand(a.clips, n, device="cuda:0") * 2 - 1
    nbytes = x.numel() * 4
    if a.case in ("rms_general", "zcr_general"):
        os.environ["SMX_DISABLE_FAST"] = "1"
    if a.case in ("rms", "rms_general"):
        run = lambda: S.rms(x, fl, hop)
    elif a.case in ("zcr", "zcr_general"):
        run = lambda: S.zero_crossing_rate(x, fl, hop)
    elif a.case == "power":
        c = Stft.Config.create(fft_size=fl, hop=hop)
        run = lambda: Stft.power_spectrum(c, x, 1.0)
    elif a.case == "compose":
        run = lambda: F.pad(x, (fl // 2, fl // 2)).double().unfold(-1, fl, hop).square().mean(dim=-1).sqrt().float()
    elif a.case == "rms_spectrogram":
        s = Stft.power_spectrum(Stft.Config.create(fft_size=fl, hop=hop), x, 1.0)
        del x
        nbytes = s.numel() * 4
        run = lambda: S.rms_of_spectrogram(s, fl)
    elif a.case == "stage_step":
        chunk = x[:, :4096].contiguous()
        nbytes = chunk.numel() * 4
        stage = S.rms_stage(fl, hop)
        stage.step(chunk)
        run = lambda: stage.step(chunk)
    else:
        raise SystemExit("unknown case %s" % a.case)
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
    line = {"case": a.case, "rate": a.rate, "clips": a.clips, "samples": n, "frames": energy.frames(n, fl, hop), "steps": a.steps,
            "inner": a.inner, "ms_median": round(times[len(times) // 2], 4), "ms_min": round(times[0], 4), "ms_max": round(times[-1], 4),
            "input_bytes": nbytes, "ms_one_read_at_8TBs": round(nbytes / PEAK_BYTES_PER_S * 1e3, 4)}
    print(json.dumps(line))


if __name__ == "__main__":
    main()
