"""Device time of nmf and nmf_activations, float32, device-resident in and out: HIP events around one call of --rounds rounds, the
median over --steps calls after --warmup, per call and per round.  One case per process, so that a launcher can give each its own
time limit:

    for b in frobenius kullback-leibler; do for k in 8 16 32 64; do for c in nmf compose; do
        timeout -k 10 300 python tools/bench_decompose.py --case $c --beta $b --k $k || break 3
    done; done; done

    --shape c2      256 clips x 1025 x 431: the magnitude spectrogram of 10 s at 22050 Hz, fft 2048, hop 512
            one     one clip of it
            custom  --clips --f --t
    nmf                  the flat function: the tile route for K <= 64
    nmf_general          the general kernels (SMX_DISABLE_FAST)
    activations_shared   nmf_activations against one dictionary [F; K] for the batch
    compose              the same updates composed in torch (matmul on batches, float32) on the same device -- what a user would
                         write today
    floor                no device work: a round reads V twice (--hbm bytes per second) and does its products, 4 F T K flops per clip
                         and round for Frobenius and 8 F T K for Kullback-Leibler, at --mfma-rate (the float32 matrix rate)

V is a rank-8 product plus noise.  Each line is JSON: median / min / max milliseconds per call and the median per round."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"c2": (256, 1025, 431), "one": (1, 1025, 431)}
EPS = 2.0 ** -23


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", required=True)
    ap.add_argument("--shape", default="c2")
    ap.add_argument("--beta", default="frobenius")
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=100)
    ap.add_argument("--clips", type=int, default=1)
    ap.add_argument("--f", type=int, default=1025)
    ap.add_argument("--t", type=int, default=431)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--mfma-rate", type=float, default=1.55e14)
    ap.add_argument("--hbm", type=float, default=8e12)
    a = ap.parse_args()

    clips, F, T = SHAPES[a.shape] if a.shape in SHAPES else (a.clips, a.f, a.t)
    K, kl = a.k, a.beta == "kullback-leibler"
    line = {"case": a.case, "shape": a.shape, "beta": a.beta, "clips": clips, "F": F, "T": T, "K": K, "rounds": a.rounds}
    if a.case == "floor":
        flops = (8 if kl else 4) * clips * F * T * K
        line.update({"ms_floor_traffic_per_round": round(2 * clips * F * T * 4 / a.hbm * 1e3, 4),
                     "ms_floor_products_per_round": round(flops / a.mfma_rate * 1e3, 4)})
        print(json.dumps(line))
        return

    import torch
    import soundml_amd as S

    torch.manual_seed(0)
    dev = "cuda:0"
    V = (torch.rand(clips, F, 8, device=dev) ** 3 @ torch.rand(clips, 8, T, device=dev) ** 2 + 0.01 * torch.rand(clips, F, T, device=dev)).contiguous()
    W0, H0 = 1.0 - torch.rand(clips, F, K, device=dev), 1.0 - torch.rand(clips, K, T, device=dev)
    case = a.case
    if case.endswith("_general"):
        os.environ["SMX_DISABLE_FAST"] = "1"
        case = case[:-len("_general")]
    if case == "nmf":
        run = lambda: S.nmf(V, K, n_iter=a.rounds, beta=a.beta, W0=W0, H0=H0)
    elif case == "activations_shared":
        D = W0[0].contiguous()
        run = lambda: S.nmf_activations(V, D, n_iter=a.rounds, beta=a.beta, H0=H0)
    elif case == "compose":
        def run():
            W, H = W0, H0
            for _ in range(a.rounds):
                if kl:
                    R = V / (W @ H).clamp_min(EPS)
                    H = H * (W.mT @ R) / W.sum(-2)[..., None].clamp_min(EPS)
                    R = V / (W @ H).clamp_min(EPS)
                    W = W * (R @ H.mT) / H.sum(-1)[..., None, :].clamp_min(EPS)
                else:
                    H = H * (W.mT @ V) / ((W.mT @ W) @ H).clamp_min(EPS)
                    W = W * (V @ H.mT) / (W @ (H @ H.mT)).clamp_min(EPS)
            return W, H
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
    line.update({"steps": a.steps, "ms_median": round(med, 4), "ms_min": round(times[0], 4), "ms_max": round(times[-1], 4),
                 "ms_per_round": round(med / max(1, a.rounds), 5)})
    print(json.dumps(line))


if __name__ == "__main__":
    main()
