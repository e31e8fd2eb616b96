"""Loudness on the device against the numpy restatement (tests/loudness_restatement.py; test_loudness_restatement.py holds that to
EBU Tech 3341): block energies bit for bit on every face and both routes, the loudness faces within one float32 ulp of the
restatement evaluated on the same energies (the device's log10 is not numpy's), the gates' verdict block by block, the EBU signals
at full length, true peak bit for bit, normalize."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from soundml_amd import Iir, Loudness
from conftest import ROOT

import loudness_restatement as R

pytestmark = pytest.mark.gpu

B, W = Iir.BLOCK, Iir.SPAN_BLOCKS
# (rate, n): at 48000 a step is 4800 = 18 blocks + 192 samples, so step edges cut Iir blocks; the last n of each rate crosses a wave's
# span (W B = 16384 samples) and leaves a tail for the general kernel; 11025 has the odd step 1103
SIZES = [(48000, 19199), (48000, 19200), (48000, 19201), (48000, 48000 + 777), (48000, 2 * W * B + 4800 * 3 + 5),
         (44100, W * B + 4410 * 3 + 5), (22050, W * B + 2205 * 3 + 5), (8000, W * B + 7), (11025, W * B + 1103 * 2 + 5)]
CHANNELS = [1, 2, 5]
CLIPS = 3


def device(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)


def same(got, want, what):
    got, want = np.ascontiguousarray(host(got)), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    word = {4: np.int32, 8: np.int64, 1: np.uint8}[want.dtype.itemsize]
    differ = got.view(word) != want.view(word)
    assert not differ.any(), "%s: %d/%d values differ, the first at %d (%r, expected %r)" % (
        what, int(differ.sum()), differ.size, int(np.argmax(differ)), got.reshape(-1)[np.argmax(differ)], want.reshape(-1)[np.argmax(differ)])


def within_one_float32_ulp(got, want, what):
    """want float64 from the restatement; -inf must be -inf"""
    got, want = host(got).astype(np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert not np.isnan(got).any(), what
    inf = np.isneginf(want)
    assert np.array_equal(np.isneginf(got), inf), what
    err = np.abs(got[~inf] - want[~inf])
    ulp = np.spacing(np.abs(want[~inf]).astype(np.float32)).astype(np.float64)
    print("%s: largest error %.3g float32 ulp" % (what, float((err / ulp).max()) if err.size else 0.0))
    assert np.all(err <= ulp), "%s: %d values off by more than one float32 ulp (worst %.3g ulp)" % (what, int((err > ulp).sum()), float((err / ulp).max()))


@functools.lru_cache(maxsize=None)
def case(rate, n, channels, wide=False):
    """the batch and what the restatement makes of it; wide: float64 samples that float32 cannot hold"""
    x = R.noise(1000 + channels, CLIPS, channels, n)
    if wide:
        x = x.astype(np.float64) * (1.0 + 2.0 ** -30)
        x.setflags(write=False)
    return x, R.measure(x, rate)


@pytest.mark.parametrize("channels", CHANNELS)
@pytest.mark.parametrize("rate,n", SIZES)
def test_block_energy_bits(rate, n, channels):
    x, m = case(rate, n, channels)
    same(Loudness.block_energy(device(x), rate), m.z, "device float32")
    same(Loudness.block_energy(x, rate), m.z, "host float32")
    same(Loudness.block_energy(device(x[0]), rate), m.z[0], "device float32, the first clip alone")   # lead (): a leading slice of the batch
    same(Loudness.block_energy(device(x[:2]), rate), m.z[:2], "device float32, a leading slice")


@pytest.mark.parametrize("rate,n", [SIZES[3], SIZES[4], SIZES[8]])
def test_block_energy_bits_float64_host(rate, n):
    x, m = case(rate, n, 2, True)
    same(Loudness.block_energy(x, rate), m.z, "host float64")
    same(Loudness.block_energy(x[0], rate), m.z[0], "host float64, the first clip alone")


CHILD = r"""
import sys
import numpy as np
import torch
sys.path[:0] = [sys.argv[2], sys.argv[3]]
from soundml_amd import Loudness
import loudness_restatement as R
out = {}
for key in sys.argv[4:]:
    rate, n, channels = (int(v) for v in key.split("_"))
    x = R.noise(1000 + channels, 3, channels, n)
    out["d_" + key] = Loudness.block_energy(torch.from_numpy(np.ascontiguousarray(x)).cuda(), rate).cpu().numpy()
    out["h_" + key] = Loudness.block_energy(x.astype(np.float64) * (1.0 + 2.0 ** -30), rate)
    out["i_" + key] = Loudness.integrated(torch.from_numpy(np.ascontiguousarray(x)).cuda(), rate).cpu().numpy()
np.savez(sys.argv[1], **out)
"""


def test_general_kernel_gives_the_same_bits(tmp_path):
    """SMX_DISABLE_FAST=1 in a child process: everything through the general kernel"""
    picks = [(48000, 48000 + 777, 2), (48000, 2 * W * B + 4800 * 3 + 5, 5), (11025, W * B + 1103 * 2 + 5, 1)]
    keys = ["%d_%d_%d" % p for p in picks]
    path = str(tmp_path / "general.npz")
    env = dict(os.environ, SMX_DISABLE_FAST="1")
    done = subprocess.run([sys.executable, "-c", CHILD, path, ROOT, os.path.join(ROOT, "tests")] + keys, env=env, capture_output=True, text=True, timeout=300)
    assert done.returncode == 0, done.stderr[-2000:]
    got = np.load(path)
    for (rate, n, channels), key in zip(picks, keys):
        same(got["d_" + key], case(rate, n, channels)[1].z, "general kernel, device float32 " + key)
        if channels == 2:
            same(got["h_" + key], case(rate, n, channels, True)[1].z, "general kernel, host float64 " + key)
        same(got["i_" + key], host(Loudness.integrated(device(case(rate, n, channels)[0]), rate)), "integrated, general kernel against block route " + key)


LONG = [(8000, 4 * 8000 + 777), (48000, 31 * 4800 + 777)]          # 37 and 28 blocks: short-term windows exist


@pytest.mark.parametrize("rate,n", LONG)
def test_loudness_faces(rate, n):
    weights = (1.0, 0.5)
    x = R.noise(5, CLIPS, 2, n) * np.array([1.0, 0.05, 1e-3], np.float32)[:, None, None]
    m = R.measure(x, rate, weights)
    assert m.short_term.shape[-1] == R.blocks(rate, n) - 26 >= 2
    for name, arg in (("device", device(x)), ("host", x)):
        within_one_float32_ulp(Loudness.momentary(arg, rate, weights=weights), m.momentary, name + " momentary")
        within_one_float32_ulp(Loudness.short_term(arg, rate, weights=weights), m.short_term, name + " short_term")
        within_one_float32_ulp(Loudness.integrated(arg, rate, weights=weights), m.integrated, name + " integrated")
    wide = x.astype(np.float64) * (1.0 + 2.0 ** -30)
    m = R.measure(wide, rate, weights)
    for got, want in ((Loudness.momentary(wide, rate, weights=weights), m.momentary), (Loudness.short_term(wide, rate, weights=weights), m.short_term),
                      (Loudness.integrated(wide, rate, weights=weights), m.integrated)):
        assert got.dtype == np.float64 and got.shape == want.shape
        live = np.isfinite(want)
        assert np.array_equal(got[~live], want[~live]) and np.abs(got[live] - want[live]).max() <= 1e-12


def test_gating():
    """three levels: each gate drops blocks, none within a factor 1.001 of a threshold (checked by the restatement), and the
    device's verdict equals the restatement's block by block"""
    x = R.gating_clip()
    m = R.measure(x, 48000)
    e = m.e[0]
    first, both, want = R.gates(e)
    assert (~first).sum() >= 1 and (first & ~both).sum() >= 1 and both.sum() >= 1
    for threshold in (R.E_ABS, 0.1 * R.serial_mean(e[first])):
        assert not np.any((e / threshold > 1 / 1.001) & (e / threshold < 1.001))
    same(Loudness.gate_mask(device(x), 48000), m.mask, "device mask")
    same(Loudness.gate_mask(x, 48000), m.mask, "host mask")
    within_one_float32_ulp(Loudness.integrated(device(x), 48000), m.integrated, "gated integrated")


def test_silence_gives_minus_infinity_and_never_nan():
    n = 48000 + 777
    x = np.zeros((2, 2, n), np.float32)
    for arg in (device(x), x):
        assert np.all(np.isneginf(host(Loudness.integrated(arg, 48000))))
        assert np.all(np.isneginf(host(Loudness.momentary(arg, 48000))))
        assert np.all(host(Loudness.block_energy(arg, 48000)) == 0)
    y = np.array(R.noise(9, 2, 2, n))
    y[:, 1] = 0.0                                            # an all-zero channel beside a live one
    m = R.measure(y, 48000)
    got = host(Loudness.integrated(device(y), 48000))
    assert np.all(np.isfinite(got))
    within_one_float32_ulp(got, m.integrated, "a silent channel")
    within_one_float32_ulp(Loudness.momentary(device(y), 48000, weights=(0.0, 1.0)), np.full(m.momentary.shape, -np.inf), "the live channel dropped")


@pytest.mark.parametrize("k", sorted(R.EBU))
def test_ebu_3341_on_the_device(k):
    _, weights, want = R.EBU[k]
    got = float(Loudness.integrated(device(R.ebu_signal(k)), R.EBU_RATE, weights=weights))
    print("EBU Tech 3341 case %d: %.4f LUFS on the device (expected %.1f)" % (k, got, want))
    assert abs(got - want) <= 0.1


@pytest.mark.parametrize("n", [1, 11, 12, 13, 4800, 4 * 1024 * 4 + 3])
def test_true_peak_bits(n):
    """history shorter than the filter, a span edge; the max is exact in any order"""
    h = Loudness.true_peak_taps()
    x = R.noise(21, CLIPS, 2, n)
    want = R.true_peak(x.reshape(-1, n), h).reshape(CLIPS, 2)
    same(Loudness.true_peak(device(x)), want.astype(np.float32), "device float32")
    same(Loudness.true_peak(x), want.astype(np.float32), "host float32")
    wide = x.astype(np.float64) * (1.0 + 2.0 ** -30)
    same(Loudness.true_peak(wide), R.true_peak(wide.reshape(-1, n), h).reshape(CLIPS, 2), "host float64")
    same(Loudness.true_peak(device(x[0, :, 1:])), R.true_peak(x[0, :, 1:], h).astype(np.float32), "rows that start off a 16-byte boundary")


def test_true_peak_of_the_ebu_tones():
    x = np.stack([R.tone(k) for k in range(len(R.TONES))])[:, None, :]
    got = 20.0 * np.log10(host(Loudness.true_peak(device(x))).astype(np.float64)[:, 0])
    for k, (_, _, _, want) in enumerate(R.TONES):
        print("tone %d: %.4f dBTP on the device (expected %.1f)" % (k, got[k], want))
        assert want - 0.4 <= got[k] <= want + 0.2


def test_normalize():
    rate, n = 48000, 48000 + 777
    x = np.array(R.noise(31, 4, 2, n)) * np.array([1.0, 0.2, 3.0, 0.0], np.float32)[:, None, None]      # the last clip is silent
    m = R.measure(x, rate)
    peaks = R.true_peak(x.reshape(-1, n), Loudness.true_peak_taps()).reshape(4, 2)
    for ceiling in (None, 0.1):
        gains = np.array([R.gain(m.integrated[c], peaks[c], -23.0, ceiling) for c in range(4)])
        want = gains[:, None, None] * x.astype(np.float64)
        for arg in (device(x), x):
            got = host(Loudness.normalize(arg, rate, target=-23.0, peak_ceiling=ceiling))
            assert got.dtype == np.float32
            within_one_float32_ulp(got, want, "normalize (ceiling %s)" % ceiling)
            same(got[3], x[3], "the silent clip")
        out = Loudness.normalize(device(x), rate, target=-23.0, peak_ceiling=ceiling)
        loud = host(Loudness.integrated(out, rate)).astype(np.float64)
        if ceiling is None:
            assert np.abs(loud[:3] + 23.0).max() <= 1e-3
        else:
            assert gains[2] < R.gain(m.integrated[2], None) and np.all(loud[:3] <= -23.0 + 1e-3)      # the ceiling binds on the loud clip
            assert float(host(Loudness.true_peak(out)).max()) <= ceiling * (1.0 + 1e-6)
