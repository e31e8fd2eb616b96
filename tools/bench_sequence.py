"""Device time of dtw, dtw_distance and cost_matrix, float32, device-resident in and out: HIP events around --inner calls in a
row, the median over --steps such windows after --warmup, per call.  One case per process, so that a launcher can give each its
own time limit:

    for s in c2 c2d20 long; do for c in dtw dtw_distance cost_matrix dtw_general dtw_distance_general cost_matrix_general compose floor; do
        timeout -k 10 300 python tools/bench_sequence.py --shape $s --case $c || break 2
    done; done

    --shape c2      256 pairs x 12 x 431 x 431: chroma of 10 s at 22050 Hz, hop 512
            c2d20   the same at d = 20 (MFCC)
            long    one pair of 12 x 4096 x 4096
            custom  --pairs --d --n --m (the sweep that places the route table's line)
    dtw / dtw_distance / cost_matrix   the flat functions: the tile route where the route table sends the shape
    *_general                          the general kernels (SMX_DISABLE_FAST)
    compose                            the same D composed in torch on the same device: torch.cdist in float64, then one
                                       minimum / add round per anti-diagonal -- what a user would write today
    floor                              no device work: the cost scratch written and read once (8 + 8 bytes a cell) plus D written
                                       (4 bytes a cell) at --hbm bytes per second, and the feature products, pairs n m d
                                       multiply-adds, over --fma-rate (profiles/pitch/NOTES.md: 3.66e13 measured); the chains are
                                       a difference, a product and a sum each, so their own floor is three times that

The features are uniform noise; Y is X's frames resampled to m with noise added.  Each line is JSON: median / min / max
milliseconds per call."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"c2": (256, 12, 431, 431), "c2d20": (256, 20, 431, 431), "long": (1, 12, 4096, 4096)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", required=True)
    ap.add_argument("--shape", default="c2")
    ap.add_argument("--pairs", type=int, default=1)
    ap.add_argument("--d", type=int, default=12)
    ap.add_argument("--n", type=int, default=431)
    ap.add_argument("--m", type=int, default=0)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--fma-rate", type=float, default=3.66e13)
    ap.add_argument("--hbm", type=float, default=8e12)
    a = ap.parse_args()

    pairs, d, n, m = SHAPES[a.shape] if a.shape in SHAPES else (a.pairs, a.d, a.n, a.m or a.n)
    line = {"case": a.case, "shape": a.shape, "pairs": pairs, "d": d, "n": n, "m": m}
    if a.case == "floor":
        cells = pairs * n * m
        line.update({"cells": cells, "ms_floor_traffic": round(cells * 20 / a.hbm * 1e3, 4), "ms_floor_products_fused": round(cells * d / a.fma_rate * 1e3, 4),
                     "ms_floor_products_as_stated": round(3 * cells * d / a.fma_rate * 1e3, 4)})
        print(json.dumps(line))
        return

    import torch
    import soundml_amd as S

    torch.manual_seed(0)
    X = torch.rand(pairs, d, n, device="cuda:0")
    at = torch.linspace(0, n - 1, m, device="cuda:0").round().long()
    Y = (X[:, :, at] + 0.05 * torch.rand(pairs, d, m, device="cuda:0")).contiguous()
    case = a.case
    if case.endswith("_general"):
        os.environ["SMX_DISABLE_FAST"] = "1"
        case = case[:-len("_general")]
    if case == "dtw":
        run = lambda: S.dtw(X, Y)
    elif case == "dtw_distance":
        run = lambda: S.dtw_distance(X, Y)
    elif case == "cost_matrix":
        run = lambda: S.cost_matrix(X, Y)
    elif case == "compose":
        ar = torch.arange(max(n, m), device="cuda:0")

        def run():
            C = torch.cdist(X.transpose(1, 2).double(), Y.transpose(1, 2).double())
            D = torch.full((pairs, n + 1, m + 1), float("inf"), dtype=torch.float64, device="cuda:0")
            D[:, 0, 0] = 0.0
            for g in range(n + m - 1):
                i = ar[max(0, g - m + 1):min(n - 1, g) + 1]
                j = g - i
                best = torch.minimum(torch.minimum(D[:, i, j], D[:, i + 1, j]), D[:, i, j + 1])
                D[:, i + 1, j + 1] = C[:, i, j] + best
            return D[:, 1:, 1:].float()
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
