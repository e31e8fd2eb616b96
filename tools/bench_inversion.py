"""Device time of Mel.invert (200 rounds) and mel_to_audio on 256 clips x 10 s at 22050 Hz (128 mels x 431 frames per clip at
fft 2048 / hop 512), float32, device-resident in and out: HIP events around --inner calls in a row, the median over --steps such
windows after --warmup, per call.  One case per process, so that a launcher can give each its own time limit:

    for c in invert invert_general compose griffin_lim mel_to_audio; do
        timeout -k 10 300 python tools/bench_inversion.py --case $c || break
    done

    invert          Mel.invert on the resident mel spectrogram: the wave kernel, one launch
    invert_general  the same with SMX_DISABLE_FAST: a workgroup per frame over scratch memory
    compose         yardstick: the same iteration in torch, two dense matmuls per round (W y - m, W^T r), relu, momentum
    griffin_lim     Stft.griffin_lim (32 rounds) on the magnitudes mel_to_stft made
    mel_to_audio    mel_to_stft + griffin_lim end to end

Each line is JSON (appended to --out as well): median / min / max milliseconds per call, and for the solver its two floors,
computed: one read of m plus one write of s at the data sheet's 8 TB/s, and the LDS words the rows' gathers read (2 nnz(W) per
round and frame) at the 75 TB/s all compute units reach together with 4-byte LDS reads."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK_BYTES_PER_S = 8e12
LDS_B32_BYTES_PER_S = 75e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", required=True)
    ap.add_argument("--rate", type=int, default=22050)
    ap.add_argument("--clips", type=int, default=256)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--n-iter", type=int, default=200)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--inner", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "inversion", "bench_inversion.jsonl"))
    a = ap.parse_args()

    import numpy as np
    import torch
    import soundml_amd as S
    from soundml_amd import Mel, Stft

    torch.manual_seed(0)
    fft, hop, n_mels, n = 2048, 512, 128, int(a.rate * a.seconds)
    sc = Stft.Config.create(fft_size=fft, hop=hop)
    mc = Mel.Config.create(n_mels, a.rate, fft)
    x = torch.rand(a.clips, n, device="cuda:0") * 2 - 1
    m = S.mel_spectrogram(sc, mc, x)
    del x
    frames = int(m.shape[-1])
    w64 = Mel.filterbank(np.float64, mc)
    nnz = int((w64 != 0.0).sum())
    extra = {}
    if a.case == "invert_general":
        os.environ["SMX_DISABLE_FAST"] = "1"
    if a.case in ("invert", "invert_general"):
        run = lambda: Mel.invert(mc, m, a.n_iter)
        moved = (m.numel() + a.clips * mc.bins * frames) * 4
        lds = 2 * nnz * 4 * a.n_iter * a.clips * frames
        extra = {"bytes_m_plus_s": moved, "ms_memory_floor_at_8TBs": round(moved / PEAK_BYTES_PER_S * 1e3, 4), "nnz": nnz,
                 "lds_bytes_read": lds, "ms_lds_floor_at_75TBs": round(lds / LDS_B32_BYTES_PER_S * 1e3, 4)}
    elif a.case == "compose":
        w = torch.from_numpy(w64).to("cuda:0", torch.float32)
        wt = w.t().contiguous()
        eta = float(1.0 / np.abs(w64 @ w64.T).sum(axis=1).max())

        def run():
            s = torch.zeros(a.clips, mc.bins, frames, device="cuda:0")
            y = s
            t = 1.0
            for _ in range(a.n_iter):
                nxt = (1.0 + (1.0 + 4.0 * t * t) ** 0.5) / 2.0
                g = torch.matmul(wt, torch.matmul(w, y) - m)
                sn = torch.relu(y - eta * g)
                y = sn + ((t - 1.0) / nxt) * (sn - s)
                s, t = sn, nxt
            return s
    elif a.case == "griffin_lim":
        mag = S.mel_to_stft(mc, m, n_iter=a.n_iter)
        run = lambda: Stft.griffin_lim(sc, mag)
    elif a.case == "mel_to_audio":
        run = lambda: S.mel_to_audio(sc, mc, m, n_iter=a.n_iter)
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
    line = {"case": a.case, "rate": a.rate, "clips": a.clips, "n_mels": n_mels, "bins": mc.bins, "frames": frames, "n_iter": a.n_iter,
            "steps": a.steps, "inner": a.inner, "ms_median": round(times[len(times) // 2], 4), "ms_min": round(times[0], 4),
            "ms_max": round(times[-1], 4)}
    line.update(extra)
    text = json.dumps(line)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
