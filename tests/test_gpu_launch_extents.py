"""Every device face whose launch limit small inputs can reach, one clip range past that limit (DESIGN.md "Launch extents").

One launch holds at most 2^32 - 1 work-items along x and 65535 slices along y or z; a launcher whose batch exceeds that goes clip
range by clip range, and the law is that the batch's result is bit for bit the concatenation of its ranges' results, wherever they are
cut.  Each test follows test_gpu_parity.test_generic_route_beyond_65535_clips:

  * ELEVEN distinct tiny clips, repeated ON THE DEVICE to L = (the largest single launch) + 8 clips, so that the second range holds 8
    clips.  11 divides none of 65535, 4194303, 16777215 (7 divides 2^24 - 1 = 16777215), so the second range starts in the middle of the
    pattern: a range that restarted at clip 0 of its input, output or scratch would land on another clip of the pattern;
  * the first 11 results against the module's own reference at the module's own tolerance (named at each test);
  * all L results against those 11, tiled, by torch.equal on their int32 words on the device: nothing of size L reaches the host.

What each test would catch in its launcher: the last clip of range 1 and the first of range 2 swapped or skipped (the tiled
comparison across the cut), a range's input, output or scratch offset dropped (range 2 would repeat the pattern from its clip 0, or
leave its outputs unwritten), and, for
mfcc, the call-wide maximum taken per range (the loudest clip sits in range 2 only).

Each test prints its wall time and torch's peak allocation (profiles/launch_extents/NOTES.md keeps them)."""
import contextlib
import os
import time

import numpy as np
import pytest
import torch

import soundml_amd as S
from soundml_amd import Mel, Stft, Window, onset
from oracle import soundml_oracle as O

import contrast_onset_restatement as CR
import energy_restatement as ER
import inversion_restatement as IR
import rhythm_restatement as RR
import sequence_restatement as SR

pytestmark = pytest.mark.gpu

PERIOD = 11
X256 = (2 ** 32 - 1) // 256        # 16 777 215 workgroups of 256: the largest single launch
X1024 = (2 ** 32 - 1) // 1024      # 4 194 303 workgroups of 1024
YZ = 65535                         # slices on grid.y / grid.z
assert all(limit % PERIOD for limit in (X256, X1024, YZ))


@contextlib.contextmanager
def general_route():
    """SMX_DISABLE_FAST is read per call (test_gpu_iir.route)"""
    saved = os.environ.get("SMX_DISABLE_FAST")
    os.environ["SMX_DISABLE_FAST"] = "1"
    try:
        yield
    finally:
        if saved is None:
            os.environ.pop("SMX_DISABLE_FAST", None)
        else:
            os.environ["SMX_DISABLE_FAST"] = saved


@contextlib.contextmanager
def measured(what):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    yield
    torch.cuda.synchronize()
    print("\nlaunch-extents %-44s %6.2f s  peak %7.1f MiB" % (what, time.perf_counter() - t0, torch.cuda.max_memory_allocated() / 2.0 ** 20))


def distinct(a):
    """the pattern holds PERIOD clips of which no two are equal"""
    a = np.ascontiguousarray(a)
    assert a.shape[0] == PERIOD and len(np.unique(a.reshape(PERIOD, -1), axis=0)) == PERIOD
    return a


def batch(pattern, L):
    """L clips on the device: the pattern repeated, cut at L"""
    t = torch.from_numpy(distinct(pattern)).cuda()
    return t.repeat((L + PERIOD - 1) // PERIOD, *([1] * (t.dim() - 1)))[:L].contiguous()


def words(t):
    return t.contiguous().reshape(t.shape[0], -1).view(torch.int32)


def every_clip_is_its_pattern(got, L, what):
    """clip i of the result is clip i % PERIOD of it, bit for bit, on the device"""
    assert got.is_cuda and got.shape[0] == L, (what, tuple(got.shape))
    w = words(got)
    whole = L // PERIOD * PERIOD
    head = w[:PERIOD]
    assert torch.equal(w[:whole].reshape(-1, PERIOD, w.shape[1]), head.unsqueeze(0).expand(whole // PERIOD, -1, -1)), what
    assert torch.equal(w[whole:], head[:L - whole]), what + ": the last clips"


def same_bits(gotp, want, what):
    gotp = gotp.cpu().numpy()
    assert gotp.shape == want.shape and gotp.dtype == want.dtype, (what, gotp.shape, gotp.dtype, want.shape, want.dtype)
    assert np.array_equal(np.ascontiguousarray(gotp).view(np.int32), np.ascontiguousarray(want).view(np.int32)), what


# ---- Energy: energy_frames_general_kernel, rms_of_spectrogram_kernel (256 threads a tile) -----------------------------------------

def energy_pattern():
    return ER.decades(12, PERIOD, 2, np.float32)            # test_gpu_energy's generator: noise scaled over 12 decades 


@pytest.mark.parametrize("L", [X256, X256 + 8], ids=["the-largest-single-launch", "a-second-range-of-8"])
def test_rms(L):
    """frame_length 2, hop 1, two samples: three frames, one tile of the general kernel per clip.  Bit for bit against the kernel-order
    restatement, as test_gpu_energy.test_bit_for_bit_against_the_kernel_order.  L = 16 777 215 pins the boundary itself."""
    xp = energy_pattern()
    with measured("rms L=%d" % L):
        got = S.rms(batch(xp, L), 2, 1)
        assert tuple(got.shape) == (L, 1, 3)
        same_bits(got[:PERIOD], ER.rms_kernel_order(xp, 2, 1), "rms")
        every_clip_is_its_pattern(got, L, "rms")


def test_zero_crossing_rate():
    """as test_rms; the restatement's bits (test_gpu_energy)"""
    L = X256 + 8
    xp = energy_pattern()
    want = ER.zcr_kernel_order(xp, 2, 1)
    crossing = want.reshape(PERIOD, 3)[:, 1] == 0.5             # the middle frame holds both samples
    assert 3 <= int(crossing.sum()) <= PERIOD - 3 and not want.reshape(PERIOD, 3)[:, ::2].any()
    with measured("zero_crossing_rate L=%d" % L):
        got = S.zero_crossing_rate(batch(xp, L), 2, 1)
        assert tuple(got.shape) == (L, 1, 3)
        same_bits(got[:PERIOD], want, "zero_crossing_rate")
        every_clip_is_its_pattern(got, L, "zero_crossing_rate")


def test_rms_of_spectrogram():
    """frame_length 2: two bins, one frame.  Bit for bit against the ordered restatement (test_gpu_energy.test_rms_of_spectrogram_bit_for_bit)"""
    L = X256 + 8
    sp = np.abs(ER.decades(PERIOD + 1, PERIOD, 2, np.float32)).reshape(PERIOD, 2, 1)
    with measured("rms_of_spectrogram L=%d" % L):
        got = S.rms_of_spectrogram(batch(sp, L), 2)
        assert tuple(got.shape) == (L, 1, 1)
        same_bits(got[:PERIOD], ER.rms_of_spectrogram_ordered(sp, 2), "rms_of_spectrogram")
        every_clip_is_its_pattern(got, L, "rms_of_spectrogram")


# ---- spectral_kernel: Q = 4 (centroid, flatness) and Q = 1 (roll-off), 256 threads either way ----------------------------------------

@pytest.mark.parametrize("feature", ["centroid", "rolloff", "flatness"])
def test_spectral(feature):
    """[L, 2, 1], the smallest shape of test_gpu_parity.test_spectral_vs_oracle, its magnitudes (|standard normal|) and its float32
    tolerances: rtol 2e-6 and atol 1e-7 of the peak; the roll-off is a bin frequency and exact."""
    L = X256 + 8
    sp = np.abs(np.random.default_rng(PERIOD).standard_normal((PERIOD, 2, 1))).astype(np.float32)
    fn = {"centroid": lambda M, a: M.spectral_centroid(a, sample_rate=22050),
          "rolloff": lambda M, a: M.spectral_rolloff(a, sample_rate=22050, roll_percent=0.5),   # (0.85 of two bins is the upper one for every clip here)
          "flatness": lambda M, a: M.spectral_flatness(a)}[feature]
    want = fn(O, sp)
    assert len(np.unique(want)) > 1
    with measured("spectral_%s L=%d" % (feature, L)):
        got = fn(S, batch(sp, L))
        assert tuple(got.shape) == (L, 1, 1)
        gotp = got[:PERIOD].cpu().numpy()
        if feature == "rolloff":
            assert np.array_equal(gotp, want)
        else:
            np.testing.assert_allclose(gotp, want, rtol=2e-6, atol=1e-7 * float(np.max(want)))
        every_clip_is_its_pattern(got, L, feature)


# ---- flux_kernel (256 threads a tile) ---------------------------------------------------------------------------------------------

def test_onset_flux():
    """onset.flux is the face that reaches flux_kernel with one bin; two frames, lag 1.  The gate of test_gpu_contrast_onset.test_flux:
    within one float32 ulp + ABS of the float64 restatement."""
    from test_gpu_contrast_onset import ABS
    L = X256 + 8
    dbp = np.random.default_rng(PERIOD).uniform(-80.0, 0.0, size=(PERIOD, 1, 2)).astype(np.float32)   # test_gpu_contrast_onset.noise_db
    dbp[::2, :, 1] += 40.0                                      # risers among them: a flux that is not zero
    want = CR.flux64(dbp, 1)
    assert np.count_nonzero(want[:, 1]) >= 3 and not want[:, 0].any()
    with measured("onset flux L=%d" % L):
        got = onset.flux(batch(dbp, L), 1)
        assert tuple(got.shape) == (L, 2)
        excess = CR.within_ulp32(got[:PERIOD].cpu().numpy(), want, ABS)
        assert excess <= 0.0, "%.3g beyond 1 ulp32 + %g" % (excess, ABS)
        every_clip_is_its_pattern(got, L, "flux")


# ---- Sequence: cost_kernel<., false> (256), dtw_general_kernel (1024), dtw_end_kernel (64) ------------------------------------------

def pairs_pattern(n):
    """11 pairs of d = 1 from the restatement's generator, whose batch is a pair as drawn, one scaled by 1e-6 and one by 1e6: the batches
    of four seeds (the generator seeds on the geometry: Y is drawn longer and cut)"""
    drawn = [SR.pair_batch((1, n, n + k)) for k in range(4)]
    X = np.concatenate([x for x, _ in drawn])[:PERIOD]
    Y = np.concatenate([y[:, :, :n] for _, y in drawn])[:PERIOD]
    distinct(np.concatenate([X, Y], axis=-1))
    return np.ascontiguousarray(X), np.ascontiguousarray(Y)


def test_cost_matrix():
    """d 1, n = m = 1: one block of cost_kernel per pair.  Bit for bit against the restatement (test_gpu_sequence.test_cost_matrix)"""
    L = X256 + 8
    Xp, Yp = pairs_pattern(1)
    want = SR.cost_matrix(Xp, Yp)
    assert len(np.unique(want)) > 2
    with measured("cost_matrix L=%d" % L):
        got = S.cost_matrix(batch(Xp, L), batch(Yp, L))
        assert tuple(got.shape) == (L, 1, 1)
        same_bits(got[:PERIOD], want, "cost_matrix")
        every_clip_is_its_pattern(got, L, "cost_matrix")


@pytest.mark.parametrize("face", ["dtw_distance", "dtw"])
def test_dtw(face):
    """d 1, n = m = 2 on the general route (a pair below 32 x 32 cells): a workgroup of 1024 per pair, so 4 194 303 pairs a launch; the
    scratch of a range (the diagonals, the step codes, the reversed path) is offset range by range too.  Bit for bit against the
    restatement (test_gpu_sequence.check_dtw).  The diagonal step weighs 3: among the 11 paths are all three shapes a 2 x 2 pair has."""
    L = X1024 + 8
    Xp, Yp = pairs_pattern(2)
    steps = dict(weights_add=(0, 0, 0), weights_mul=(3, 1, 1))
    D, path, dist = SR.dtw(Xp, Yp, "euclidean", steps["weights_add"], steps["weights_mul"], False)
    assert len(np.unique(path.reshape(PERIOD, -1), axis=0)) == 3
    with measured("%s L=%d" % (face, L)):
        x, y = batch(Xp, L), batch(Yp, L)
        if face == "dtw":
            gD, gpath = S.dtw(x, y, **steps)
            assert tuple(gD.shape) == (L, 2, 2) and tuple(gpath.shape) == (L, 2, 3)
            same_bits(gD[:PERIOD], D, "D")
            same_bits(gpath[:PERIOD], path, "path")
            every_clip_is_its_pattern(gD, L, "D")
            every_clip_is_its_pattern(gpath, L, "path")
        else:
            got = S.dtw_distance(x, y, **steps)
            assert tuple(got.shape) == (L, 1)
            same_bits(got[:PERIOD], dist, "distance")
            every_clip_is_its_pattern(got, L, "distance")


# ---- tempogram_general_kernel: a workgroup of 256 per frame ---------------------------------------------------------------------------

def test_tempogram_general_route():
    """win_length 1 (the smallest: test_gpu_rhythm.test_tempogram_shapes), one frame per clip, norm off so that a clip's value is its own
    (normalised, every lag-0 value is 1).  Bit for bit against the restatement under the library's own window, as
    test_gpu_rhythm.test_tempogram_bit_for_bit_against_the_restatement."""
    L = X256 + 8
    envp = np.concatenate([RR.click_batch((1, p, 1, 8000, 500)) for p in (1, 2, 3, 4)])[:PERIOD]
    want = RR.tempogram(envp, Window.make(np.float64, "hann", 1), False)
    with general_route(), measured("tempogram (general) L=%d" % L):
        got = S.tempogram(batch(envp, L), win_length=1, norm=False)
        assert tuple(got.shape) == (L, 1, 1)
        same_bits(got[:PERIOD], want, "tempogram")
        every_clip_is_its_pattern(got, L, "tempogram")


# ---- the leading slices on grid.y: mfcc, mfcc_to_mel, the float64 Mel.apply --------------------------------------------------------

def test_mfcc():
    """fft 16 advanced by 16 on 16 samples (one frame), one mel band, one coefficient: 65543 clips, 65535 + 8.  The 80 dB clamp hangs
    under the maximum of the WHOLE call: the clips' levels span 120 dB and the loudest clip of all is the LAST one, in the second range
    only, so a maximum taken range by range would lower range 1's floor by 36 dB.  The oracle takes the 11 clips and that one; tolerance
    of test_gpu_parity.test_mfcc_vs_oracle_batch (rtol 1e-4, atol 2e-3: the log domain)."""
    L = YZ + 8
    xp = np.random.default_rng(PERIOD).uniform(-1, 1, size=(PERIOD, 16)).astype(np.float32)
    xp *= (10.0 ** (-0.6 * np.arange(PERIOD, dtype=np.float64)))[:, None].astype(np.float32)     # 12 dB apart
    loud = (xp[0] * np.float32(2.0 ** 6)).astype(np.float32)   # the loudest pattern clip, 36 dB up
    sc, mc = Stft.Config.create(fft_size=16, hop=16, alignment="left"), Mel.Config.create(n_mels=1, sample_rate=8000, fft_size=16)
    assert Stft.frames(sc, 16) == 1
    osc, omc = O.stft_config(16, hop=16, alignment="left"), O.mel_config(1, 8000, 16)
    want = O.mfcc(osc, omc, np.concatenate([xp, loud[None]]), 1, None)
    alone = O.mfcc(osc, omc, xp, 1, None)
    assert np.abs(want[:PERIOD] - alone).max() > 1.0            # the last clip's level decides the others' floor
    with measured("mfcc L=%d" % L):
        x = batch(xp, L)
        x[L - 1] = torch.from_numpy(loud).cuda()
        got = S.mfcc(sc, mc, x, n_mfcc=1)
        assert tuple(got.shape) == (L, 1, 1)
        np.testing.assert_allclose(got[:PERIOD].cpu().numpy(), want[:PERIOD], rtol=1e-4, atol=2e-3)
        np.testing.assert_allclose(got[L - 1:].cpu().numpy(), want[PERIOD:], rtol=1e-4, atol=2e-3)
        every_clip_is_its_pattern(got[:L - 1], L - 1, "mfcc")


def test_mfcc_to_mel():
    """one coefficient to one band, one frame (test_gpu_mel_invert.test_mfcc_to_mel_against_the_restatement has (1, 1)); its gate: one
    float32 ulp of the float64 restatement + 1e-11"""
    L = YZ + 8
    cp = (np.random.default_rng(PERIOD).normal(size=(PERIOD, 1, 1)) * 6.0).astype(np.float32)
    want = IR.mfcc_to_mel(cp, 1, None, 1.0)
    with measured("mfcc_to_mel L=%d" % L):
        got = S.mfcc_to_mel(batch(cp, L), 1, None, 1.0)
        assert tuple(got.shape) == (L, 1, 1)
        err = np.abs(got[:PERIOD].cpu().numpy().astype(np.float64) - want)
        assert (err <= np.spacing(want.astype(np.float32)).astype(np.float64) + 1e-11).all(), float((err / want).max())
        every_clip_is_its_pattern(got, L, "mfcc_to_mel")


def test_mel_apply_float64_kernel():
    """float32 device spectrograms under the float64 interior take mel_apply_f64_kernel with every slice of the call on grid.y (the
    host faces hand it clip units).  One band over the 3 bins of an FFT of 4, one frame; test_gpu_parity.test_mel_apply_vs_oracle's
    float32 gate, check_fast, clip by clip."""
    from test_gpu_parity import check_fast
    L = YZ + 8
    sp = np.random.default_rng(PERIOD).uniform(0, 4, size=(PERIOD, 3, 1)).astype(np.float32)    # test_mel_apply_vs_oracle's draw
    mc, oc = Mel.Config.create(n_mels=1, sample_rate=8000, fft_size=4), O.mel_config(1, 8000, 4)
    want = O.mel_apply(oc, sp)
    S.set_interior("float64")
    try:
        with measured("Mel.apply (float64 kernel) L=%d" % L):
            got = Mel.apply(mc, batch(sp, L))
            assert tuple(got.shape) == (L, 1, 1) and got.dtype == torch.float32
            for i in range(PERIOD):
                check_fast(got[i].cpu().numpy(), want[i], "mel clip %d" % i)
            every_clip_is_its_pattern(got, L, "Mel.apply")
    finally:
        S.set_interior("float32")
