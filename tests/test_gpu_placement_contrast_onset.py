"""Placement of the contrast / onset device entry points: the rules of test_gpu_placement.py (guarded arena, every output word
written, no guard word touched, bit equality with the ordinary call, the entry's own gate against the yardstick) for the
entries whose names carry the dtype last (`smx_*_dev_f32`), which that file's coverage law does not see.  This file keeps a
table and a law of its own: every name of include/soundml_amd.h matching smx_\\w+_dev_f(32|64) has a row here."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import soundml_amd as S
from soundml_amd import Mel, Stft
from soundml_amd._lib import check, lib
from conftest import ROOT
from test_gpu_placement import Region, S_OUT, S_PAD, drive, host, same      # noqa: F401  (the sentinels are the arena's)

import contrast_onset_restatement as R

pytestmark = pytest.mark.gpu

TABLE = {}              # entry point -> the tests that place it
ABS = 1e-11             # test_gpu_contrast_onset.py: 1 ulp32 + 1e-11
SR = 22050
PLACEMENTS = [(0, 0, 0), (1, 0, 1), (3, 5, 3)]       # (input offset, row pad, output offset) in elements


def row(*entries):
    def mark(fn):
        for e in entries:
            TABLE.setdefault(e, []).append(fn.__name__)
        return fn
    return mark


@pytest.fixture(autouse=True)
def _default_interior():
    S.set_interior("float32")
    yield
    S.set_interior("float32")


def call(name, *args):
    import torch
    assert name in TABLE, name
    raw = [a.ptr if isinstance(a, Region) else a for a in args]
    check(getattr(lib, name)(*raw, C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    for a in args:
        if isinstance(a, Region) and not a.output:
            a.intact()


def ulp_gate(want64, absolute):
    def gate(res, pl):
        excess = R.within_ulp32(host(res[0], np.float32, want64.shape), want64, absolute)
        assert excess <= 0.0, "%s: %.3g beyond 1 ulp32 + %g" % (pl, excess, absolute)
    return gate


@row("smx_spectral_contrast_of_spectrogram_dev_f32")
def test_contrast_of_spectrogram():
    """[2; 257; 70]: a full tile and a ragged one, an odd row count; the register lists (0.02), the bisection (0.5), and the
    three outputs (a spectrogram is one packed row per call: the row pad does not apply)"""
    rng = np.random.default_rng(21)
    s = (rng.integers(0, 12, size=(2, 257, 70)) / 11.0).astype(np.float32)
    lead, bins, frames = s.shape
    for quantile in (0.02, 0.5):
        bands = R.plan(6, 200.0, quantile, SR, 512)
        for linear, clamped, fft_size in ((1, 1, 0), (0, 1, 0), (0, 0, 512)):
            want = R.contrast64(s, bands, bool(linear), bool(clamped))

            def run(pl):
                sin, out = Region.of(s, pl[0]), Region.out(1, want.size, np.float32, pl[2])
                call("smx_spectral_contrast_of_spectrogram_dev_f32", sin, lead, bins, frames, fft_size, 6, 200.0, quantile, linear, SR,
                     clamped, out)
                return [out.collect()]
            drive(run, PLACEMENTS, ulp_gate(want, 0.0 if linear else ABS))


@row("smx_onset_flux_dev_f32")
def test_onset_flux():
    db = np.random.default_rng(22).uniform(-80.0, 0.0, size=(2, 40, 70)).astype(np.float32)
    lead, bins, frames = db.shape
    for lag in (1, 3, 70):
        want = R.flux64(db, lag)

        def run(pl):
            sin, out = Region.of(db, pl[0]), Region.out(1, want.size, np.float32, pl[2])
            call("smx_onset_flux_dev_f32", sin, lead, bins, frames, lag, out)
            return [out.collect()]
        drive(run, PLACEMENTS, ulp_gate(want, ABS))


@row("smx_spectral_contrast_dev_f32", "smx_onset_strength_dev_f32")
@pytest.mark.parametrize("fft,hop", [(2048, 512), (512, 128)])
def test_audio_faces(fft, hop):
    """rows n + pad apart from an offset: each is, bit for bit, its second stage on the device's own first stage (the spectrogram
    and mel entries have rows of their own in test_gpu_placement.py), which test_gpu_contrast_onset.py ties to the yardstick"""
    import torch
    clips, n = 2, hop * 39
    c = Stft.Config.create(fft_size=fft, hop=hop)
    mc = Mel.Config.create(n_mels=40, sample_rate=SR, fft_size=fft)
    x = np.random.default_rng(fft).uniform(-1, 1, size=(clips, n)).astype(np.float32)
    xd = torch.from_numpy(x).cuda()
    frames = Stft.frames(c, n)
    bits = lambda t: t.contiguous().view(torch.int32).reshape(1, -1)
    staged = S.spectral_contrast_of_spectrogram(Stft.power_spectrum(c, xd, 1.0), sample_rate=SR)
    mel = S.mel_spectrogram(c, mc, xd).cpu().numpy()
    want = R.envelope64(mel, 2, fft // (2 * hop))

    def contrast(pl):
        xin, out = Region.of(x, pl[0], pl[1]), Region.out(1, clips * 7 * frames, np.float32, pl[2])
        call("smx_spectral_contrast_dev_f32", c._h, xin, clips, n, n + pl[1], 6, 200.0, 0.02, 0, SR, out)
        return [out.collect()]
    drive(contrast, PLACEMENTS, lambda res, pl: same(res, [bits(staged)], ("spectral_contrast stages", pl)))

    def strength(pl):
        xin, out = Region.of(x, pl[0], pl[1]), Region.out(1, clips * frames, np.float32, pl[2])
        call("smx_onset_strength_dev_f32", c._h, mc._h, xin, clips, n, n + pl[1], 2, out)
        return [out.collect()]
    drive(strength, PLACEMENTS, ulp_gate(want, ABS))


def test_coverage_law():
    """every device entry point of the header whose name carries the dtype last runs in a row above (no GPU work)"""
    with open(os.path.join(ROOT, "include", "soundml_amd.h")) as fh:
        declared = set(re.findall(r"\b(smx_\w+_dev_f(?:32|64))\s*\(", fh.read()))
    assert len(declared) >= 4
    missing = sorted(declared - set(TABLE))
    assert not missing, "device entry points without a placement row: %s" % ", ".join(missing)
    assert not sorted(set(TABLE) - declared)
