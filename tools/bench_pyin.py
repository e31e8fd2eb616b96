"""Device time of pyin, pyin_observation and pyin_decode on 256 clips x 10 s at 22050 Hz (frame_length 2048 / hop 512, 65 .. 2093 Hz,
resolution 0.1: 602 bins, h = 50), float32, device-resident in and out: HIP events around --inner calls in a row, the median over
--steps such windows after --warmup, per call.  One case per process, so that a launcher can give each its own time limit; every
line is appended to profiles/pitch/bench_pyin.jsonl (--out):

    for c in pyin observation decode decode_one yin compose floor; do
        timeout -k 10 300 python tools/bench_pyin.py --case $c || break
    done

    pyin          the flat function on the resident audio: correlation, troughs, observation, decoder, walk back
    observation   pyin_observation alone (the float32 observation written out)
    decode        pyin_decode alone, on that observation
    decode_one    pyin_decode with one bin per lane (SMX_DISABLE_FAST): what the register run buys
    yin           yin on the same audio, for scale
    compose       the same decode composed in torch on the same device: per frame a float64 unfold of the padded delta, the product
                  with the triangle, a max and an argmax over the band, the switch, the product with the observation; then the walk
    floor         no device work: the decoder's multiply-compares (frames x 2 n_bins x (2 h + 1)) over --op-rate float64 operations
                  per second (3.66e13: tools/probes/f64_fma_rate_probe.hip)

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
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--inner", type=int, default=2)
    ap.add_argument("--op-rate", type=float, default=3.66e13)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pitch", "bench_pyin.jsonl"))
    a = ap.parse_args()

    import soundml_amd as S
    from soundml_amd import Pitch

    fl, hop, n, sr, fmin, fmax = 2048, 512, int(a.rate * a.seconds), a.rate, 65.0, 2093.0
    nb, h, count = Pitch.pyin_bins(fmin, fmax, 0.1), Pitch.pyin_half_width(sr, hop, 0.1, 35.92), Pitch.frames(n, fl, hop)
    line = {"case": a.case, "rate": a.rate, "clips": a.clips, "samples": n, "frames": count, "n_bins": nb, "half_width": h}

    def emit():
        print(json.dumps(line))
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "a") as fh:
            fh.write(json.dumps(line) + "\n")

    if a.case == "floor":
        ops = a.clips * (count - 1) * 2 * nb * (2 * h + 1)
        line.update({"multiply_compares": ops, "ops_per_s": a.op_rate, "ms_floor": round(ops / a.op_rate * 1e3, 4)})
        emit()
        return

    import torch
    import torch.nn.functional as F
    torch.manual_seed(0)
    x = torch.rand(a.clips, n, device="cuda:0") * 2 - 1
    # a third of the clips carry a gliding tone under the noise, so that the decoder has voiced stretches to follow
    t = torch.arange(n, device=x.device, dtype=torch.float64) / sr
    glide = torch.sin(2 * torch.pi * (110.0 * t + 40.0 * t * t)).float()
    x[::3] = 0.1 * x[::3] + glide
    if a.case == "decode_one":
        os.environ["SMX_DISABLE_FAST"] = "1"
    if a.case == "pyin":
        run = lambda: S.pyin(x, fmin, fmax, sr, fl, hop)
    elif a.case == "observation":
        run = lambda: S.pyin_observation(x, fmin, fmax, sr, fl, hop)
    elif a.case == "yin":
        run = lambda: S.yin(x, fmin, fmax, sr, fl, hop, 0.1, True)
    elif a.case in ("decode", "decode_one"):
        obs = S.pyin_observation(x, fmin, fmax, sr, fl, hop)
        run = lambda: S.pyin_decode(obs, h)
    elif a.case == "compose":
        obs = S.pyin_observation(x, fmin, fmax, sr, fl, hop).double().clamp_min(Pitch.OBSERVATION_FLOOR)
        tab = Pitch.pyin_tables(fmin, fmax, sr, fl, hop)
        tri = torch.from_numpy(tab["tri"]).to(x.device).flip(0)            # unfold window w holds source j - h + w: k = 2 h - w
        rs = torch.from_numpy(tab["rs"]).to(x.device)
        sp = 0.01

        def run():
            delta = torch.cat([torch.zeros(a.clips, nb, device=x.device, dtype=torch.float64),
                               torch.full((a.clips, nb), 1.0 / nb, device=x.device, dtype=torch.float64)], 1) * obs[:, :, 0]
            back = torch.empty(a.clips, count, 2 * nb, dtype=torch.int32, device=x.device)
            for f in range(1, count):
                u = (delta / delta.amax(1, keepdim=True)).view(a.clips, 2, nb) * rs
                cand = F.pad(u, (h, h)).unfold(-1, 2 * h + 1, 1) * tri
                best, arg = cand.max(-1)
                src = arg + torch.arange(nb, device=x.device) - h
                stay, change = best * (1 - sp), best.flip(1) * sp
                sw = change > stay
                delta = (torch.where(sw, change, stay) * obs[:, :, f].view(a.clips, 2, nb)).view(a.clips, 2 * nb)
                voicing = torch.tensor([0, 1], device=x.device).view(1, 2, 1)
                back[:, f] = torch.where(sw, (1 - voicing) * nb + src.flip(1), voicing * nb + src).view(a.clips, 2 * nb)
            state = delta.argmax(1)
            path = [state]
            for f in range(count - 1, 0, -1):
                state = back[:, f].gather(1, state[:, None].long())[:, 0]
                path.append(state)
            return torch.stack(path[::-1], 1)
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
    emit()


if __name__ == "__main__":
    main()
