"""Device time of tempogram, tempo and beat_track on 256 clips x 431 frames (10 s at 22050 Hz, hop 512), win_length 384, float32,
device-resident in and out: HIP events around --inner calls in a row, the median over --steps such windows after --warmup, per
call.  One case per process, so that a launcher can give each its own time limit:

    for c in tempogram tempogram_general tempo beat_track beat_track_bpm audio_to_beats compose floor; do
        timeout -k 10 300 python tools/bench_rhythm.py --case $c --fma-rate $RATE || break
    done

    tempogram / tempogram_general   the flat function on resident envelopes: the tile route, and the general one (SMX_DISABLE_FAST)
    tempo                           the float64 tempogram through scratch, the frame mean, the prior, the first argmax
    beat_track / beat_track_bpm     tempo plus the tracker, and the tracker alone at a given tempo
    audio_to_beats                  audio -> onset_strength -> beat_track, all resident
    compose                         the same tempogram composed in torch on the same device: pad, unfold, window, float64 rfft
                                    autocorrelation, normalise
    floor                           no device work: the tempogram's multiply-adds, frames x W (W + 1) / 2, over --fma-rate
                                    multiply-adds per second (profiles/pitch/NOTES.md: 3.66e13 measured); the kernel's chains
                                    are a product and a sum each, two instructions, so its own floor is twice that

The envelopes are click tracks at 123 beats per minute over noise.  Each line is JSON: median / min / max milliseconds per call."""
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
    ap.add_argument("--win-length", type=int, default=384)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--fma-rate", type=float, default=3.66e13)
    a = ap.parse_args()

    sr, hop, W, n = a.rate, 512, a.win_length, int(a.rate * a.seconds)
    frames = 1 + n // hop
    line = {"case": a.case, "clips": a.clips, "frames": frames, "win_length": W}
    if a.case == "floor":
        madds = a.clips * frames * W * (W + 1) // 2
        line.update({"madds": madds, "fma_per_s": a.fma_rate, "ms_floor_fused": round(madds / a.fma_rate * 1e3, 4),
                     "ms_floor_product_and_sum": round(2 * madds / a.fma_rate * 1e3, 4)})
        print(json.dumps(line))
        return

    import torch
    import torch.nn.functional as F
    import soundml_amd as S
    from soundml_amd import Mel, Stft

    torch.manual_seed(0)
    env = 0.05 * torch.rand(a.clips, frames, device="cuda:0")
    env[:, 3::21] += 1.0
    if a.case == "tempogram_general":
        os.environ["SMX_DISABLE_FAST"] = "1"
    if a.case in ("tempogram", "tempogram_general"):
        run = lambda: S.tempogram(env, win_length=W)
    elif a.case == "tempo":
        run = lambda: S.tempo(env, sr, hop, W)
    elif a.case == "beat_track":
        run = lambda: S.beat_track(env, sr, hop, win_length=W)
    elif a.case == "beat_track_bpm":
        run = lambda: S.beat_track(env, sr, hop, bpm=123.0, win_length=W)
    elif a.case == "audio_to_beats":
        x = torch.rand(a.clips, n, device="cuda:0") * 2 - 1
        sc, mc = Stft.Config.create(fft_size=2048, hop=hop), Mel.Config.create(n_mels=128, sample_rate=sr, fft_size=2048)
        run = lambda: S.beat_track(S.onset_strength(sc, mc, x), sr, hop, win_length=W)
    elif a.case == "compose":
        w = torch.hann_window(W, periodic=True, dtype=torch.float64, device=env.device)

        def run():
            y = F.pad(env, (W // 2, W - W // 2 - 1)).double().unfold(-1, W, 1) * w
            spec = torch.fft.rfft(y, 2 * W)
            ac = torch.fft.irfft(spec * spec.conj(), 2 * W)[..., :W]
            return (ac / ac[..., :1].clamp_min(2.3e-308)).transpose(-1, -2).float()
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
