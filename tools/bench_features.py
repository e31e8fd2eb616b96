"""Device time of onset_strength and spectral_contrast on 256 clips x 10 s (fft 2048 / hop 512, 128 mels), device-resident in
and out: HIP events around --inner calls in a row, the median over --steps such windows after --warmup, per call.  One case per
process, so that a launcher can give each its own time limit:

    for r in 22050 48000; do for c in mel onset contrast_002 contrast_linear contrast_05 contrast_general compose contrast_audio power; do
        timeout -k 10 300 python tools/bench_features.py --rate $r --case $c || break 2
    done; done

    mel               mel_spectrogram from audio alone
    onset             onset_strength from audio (the difference to `mel` is the tail: maximum, decibels, flux)
    contrast_002      spectral_contrast_of_spectrogram at quantile 0.02 (register lists in every band)
    contrast_linear   the same with linear = True: no decibels, no maxima, no second launch
    contrast_05       the same at quantile 0.5 (the bisection in every band but the lowest)
    contrast_general  quantile 0.02 with SMX_DISABLE_FAST: the bisection in every band
    compose           the same result from torch.sort per band, two means and the library's power_to_db
    power             Stft.power_spectrum (power 1) from audio alone
    contrast_audio    spectral_contrast from audio (the difference to `power` is the contrast of the spectrogram)

Each line is JSON: median / min milliseconds per call; the spectrogram cases add the bytes of one read of the spectrogram and
the time that read takes at the 8 TB/s of the data sheet (the roof of a kernel that reads every magnitude once)."""
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
    import soundml_amd as S
    from soundml_amd import Mel, Stft, contrast

    torch.manual_seed(0)
    fft, hop, n = 2048, 512, int(a.rate * a.seconds)
    c = Stft.Config.create(fft_size=fft, hop=hop)
    mc = Mel.Config.create(n_mels=128, sample_rate=a.rate, fft_size=fft)
    frames, bins = Stft.frames(c, n), fft // 2 + 1
    x = torch.rand(a.clips, n, device="cuda:0") * 2 - 1
    extra = {}
    if a.case == "mel":
        run = lambda: S.mel_spectrogram(c, mc, x)
    elif a.case == "onset":
        run = lambda: S.onset_strength(c, mc, x)
    elif a.case == "power":
        run = lambda: Stft.power_spectrum(c, x, 1.0)
    elif a.case == "contrast_audio":
        run = lambda: S.spectral_contrast(c, x, sample_rate=a.rate)
    elif a.case in ("contrast_002", "contrast_linear", "contrast_05", "contrast_general", "compose"):
        s = Stft.power_spectrum(c, x, 1.0)
        del x
        quantile = 0.5 if a.case == "contrast_05" else 0.02
        nbytes = s.numel() * 4
        extra = {"quantile": quantile, "spectrogram_bytes": nbytes, "ms_one_read_at_8TBs": round(nbytes / PEAK_BYTES_PER_S * 1e3, 4)}
        if a.case == "contrast_general":
            os.environ["SMX_DISABLE_FAST"] = "1"
        if a.case == "compose":
            bands = contrast.plan(6, 200.0, quantile, a.rate, fft)

            def run():
                valleys, peaks = [], []
                for lo, sub_len, take in bands:
                    ordered = torch.sort(s[:, lo:lo + sub_len, :], dim=1).values
                    valleys.append(ordered[:, :take].double().mean(dim=1, keepdim=True))
                    peaks.append(ordered[:, sub_len - take:].double().mean(dim=1, keepdim=True))
                valley, peak = torch.cat(valleys, dim=1).float(), torch.cat(peaks, dim=1).float()
                return S.power_to_db(peak, top_db=80.0) - S.power_to_db(valley, top_db=80.0)
        else:
            run = lambda: S.spectral_contrast_of_spectrogram(s, sample_rate=a.rate, quantile=quantile, linear=a.case == "contrast_linear")
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
    line = {"case": a.case, "rate": a.rate, "clips": a.clips, "samples": n, "frames": frames, "bins": bins, "steps": a.steps, "inner": a.inner,
            "ms_median": round(times[len(times) // 2], 4), "ms_min": round(times[0], 4), "ms_max": round(times[-1], 4)}
    line.update(extra)
    print(json.dumps(line))


if __name__ == "__main__":
    main()
