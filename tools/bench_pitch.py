"""Device time of yin and yin_difference on 256 clips x 10 s at 22050 Hz (frame_length 2048 / hop 512, 65 .. 2093 Hz), float32,
device-resident in and out: HIP events around --inner calls in a row, the median over --steps such windows after --warmup, per
call.  One case per process, so that a launcher can give each its own time limit:

    for c in yin yin_general difference compose power stage_step floor; do
        timeout -k 10 300 python tools/bench_pitch.py --case $c --fma-rate $RATE || break
    done

    yin / yin_general   the flat function on the resident audio: the tile route, and the general one (SMX_DISABLE_FAST)
    difference          yin_difference alone (the same kernels, d' written instead of the choice)
    compose             the same feature in torch on the same device: pad, unfold, float64 rfft-based correlation, cumulative sums,
                        argmax of the first trough
    power               Stft.power_spectrum on the same audio, for scale
    stage_step          one yin_stage step of 4096 samples x 256 channels in mid-stream
    floor               no device work: the definition's multiply-adds (frames x W x lags) and those the tile route runs (every
                        hop block of a tile once, lags rounded up to the 8 of a lane), over --fma-rate multiply-adds per second
                        (tools/probes/f64_fma_rate_probe.hip, measured in the same session)

Each line is JSON: median / min / max milliseconds per call."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", required=True)
    ap.add_argument("--rate", type=int, default=22050)
    ap.add_argument("--clips", type=int, default=256)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--fma-rate", type=float, default=0.0)
    ap.add_argument("--tile-frames", type=int, default=10, help="floor: frames of a tile (pitch.hip picks 10 at these shapes)")
    a = ap.parse_args()

    import torch
    import torch.nn.functional as F
    import soundml_amd as S
    from soundml_amd import Pitch, Stft

    fl, hop, n, sr, fmin, fmax, thr = 2048, 512, int(a.rate * a.seconds), a.rate, 65.0, 2093.0, 0.1
    W = fl // 2
    pmin, pmax = Pitch.lag_range(sr, fmin, fmax, fl)
    lags, count = pmax + 1, Pitch.frames(n, fl, hop)
    line = {"case": a.case, "rate": a.rate, "clips": a.clips, "samples": n, "frames": count, "lags": lags}
    if a.case == "floor":
        definition = a.clips * count * W * lags
        nf = a.tile_frames
        tiles = -(-count // nf)
        tile = a.clips * tiles * (nf + W // hop - 1) * hop * (-(-lags // 8) * 8)
        line.update({"madds_definition": definition, "madds_tile_route": tile, "fma_per_s": a.fma_rate})
        if a.fma_rate > 0:
            line.update({"ms_floor_definition": round(definition / a.fma_rate * 1e3, 4), "ms_floor_tile_route": round(tile / a.fma_rate * 1e3, 4)})
        print(json.dumps(line))
        return

    torch.manual_seed(0)
    x = torch.rand(a.clips, n, device="cuda:0") * 2 - 1
    if a.case == "yin_general":
        os.environ["SMX_DISABLE_FAST"] = "1"
    if a.case in ("yin", "yin_general"):
        run = lambda: S.yin(x, fmin, fmax, sr, fl, hop, thr, True)
    elif a.case == "difference":
        run = lambda: S.yin_difference(x, fmin, fmax, sr, fl, hop)
    elif a.case == "power":
        c = Stft.Config.create(fft_size=fl, hop=hop)
        run = lambda: Stft.power_spectrum(c, x)
    elif a.case == "compose":
        tau = torch.arange(lags, device=x.device, dtype=torch.float64)

        def run():
            fr = F.pad(x, (W, W)).double().unfold(-1, fl, hop)
            r = torch.fft.irfft(torch.fft.rfft(fr, 2 * fl) * torch.fft.rfft(fr[..., :W], 2 * fl).conj(), 2 * fl)[..., :lags]
            prefix = F.pad(torch.cumsum(fr * fr, -1), (1, 0))
            e = prefix[..., W:W + lags] - prefix[..., :lags]
            d = (e[..., :1] + e - 2 * r).clamp_min(0)
            d[..., 0] = 0
            c = torch.cumsum(d, -1)
            dn = torch.where(c > 0, d * tau / c, torch.ones_like(d))
            dn[..., 0] = 1
            mid = dn[..., pmin:lags - 1]
            trough = (mid < thr) & (mid <= dn[..., pmin - 1:lags - 2]) & (mid < dn[..., pmin + 1:])
            first = trough.to(torch.int8).argmax(-1)
            lag = torch.where(trough.any(-1), first, dn[..., pmin:].argmin(-1)) + pmin
            return (sr / lag.double()).float(), dn.gather(-1, lag[..., None])[..., 0].float()
    elif a.case == "stage_step":
        chunk = x[:, :4096].contiguous()
        stage = S.yin_stage(fmin, fmax, sr, fl, hop, thr, True)
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
    line.update({"steps": a.steps, "inner": a.inner, "ms_median": round(times[len(times) // 2], 4), "ms_min": round(times[0], 4),
                 "ms_max": round(times[-1], 4)})
    print(json.dumps(line))


if __name__ == "__main__":
    main()
