"""Placement of the inversion family's device entry points: the rules of test_gpu_placement.py (guarded arena, every output word
written, no guard word touched, inputs intact, bit equality with the ordinary call) for smx_db_to_*_dev, smx_mel_invert_*_dev and
smx_mfcc_to_mel_*_dev.  The rows register in test_gpu_placement.TABLE, so that file's coverage law counts them; the gate of each row
is the package's own call on an ordinary tensor, bit for bit (tests/test_gpu_mel_invert.py and test_gpu_convert_inverse.py hold
those to the restatement)."""
import os
import re

import numpy as np
import pytest
import torch

import soundml_amd as S
from soundml_amd import Convert, Mel
from conftest import ROOT
from test_gpu_placement import TABLE, Region, call, drive, host, row

import inversion_restatement as R

pytestmark = pytest.mark.gpu

PLACEMENTS = [(0, 0, 0), (1, 0, 1), (3, 0, 3), (2, 0, 0)]       # (input offset, -, output offset) in elements: the arrays are packed
FAMILY = r"\b(smx_(?:db_to_\w+|mel_invert|mfcc_to_mel)_f(?:32|64)_dev)\s*\("
DTYPES = {"f32": np.float32, "f64": np.float64}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def equals(want, dtype):
    want = np.ascontiguousarray(want).reshape(-1)

    def gate(res, pl):
        got = host(res[0], dtype).reshape(-1)
        assert got.shape == want.shape
        differ = got.view(np.uint8) != want.view(np.uint8)
        assert not differ.any(), "%s: differs from the package's call, the first byte at %d" % (pl, int(np.argmax(differ)))
    return gate


@row("smx_db_to_power_f32_dev", "smx_db_to_power_f64_dev", "smx_db_to_amplitude_f32_dev", "smx_db_to_amplitude_f64_dev")
@pytest.mark.parametrize("sfx", sorted(DTYPES))
@pytest.mark.parametrize("fn", ["db_to_power", "db_to_amplitude"])
@pytest.mark.parametrize("total", [1, 255, 1000])
def test_from_db(fn, sfx, total):
    dtype = DTYPES[sfx]
    db = np.linspace(-90.0, 40.0, total).astype(dtype)
    want = getattr(Convert, fn)(dev(db), reference=2.5).cpu().numpy()

    def run(pl):
        src, out = Region.of(db, pl[0]), Region.out(1, total, dtype, pl[2])
        call("smx_%s_%s_dev" % (fn, sfx), src, total, 2.5, out)
        return [out.collect()]
    drive(run, PLACEMENTS, equals(want, dtype))


@row("smx_mel_invert_f32_dev", "smx_mel_invert_f64_dev")
@pytest.mark.parametrize("route", ["wave", "general"])
@pytest.mark.parametrize("sfx", sorted(DTYPES))
@pytest.mark.parametrize("name,frames", [("fft64_mel8", 37), ("fft400_mel80", 19)])
def test_mel_invert(name, frames, sfx, route):
    """two clips whose frames share no workgroup boundary with the clips; the last workgroup of the wave kernel holds idle waves"""
    dtype = DTYPES[sfx]
    env = {"SMX_DISABLE_FAST": "1"} if route == "general" else None
    n_mels, sr, fft, scale, norm = R.BANKS[name]
    cfg = Mel.Config.create(n_mels, sr, fft, scale=scale, norm=norm)
    w = R.bank_weights(name)
    bins = w.shape[1]
    m = np.ascontiguousarray((w @ R.synthetic_spectra(bins, 2 * frames)).reshape(n_mels, 2, frames).transpose(1, 0, 2)).astype(dtype)
    for power in (1.0, 2.0):
        want = S.mel_to_stft(cfg, dev(m), power=power, n_iter=7).cpu().numpy()

        def run(pl):
            src, out = Region.of(m, pl[0]), Region.out(1, 2 * bins * frames, dtype, pl[2])
            call("smx_mel_invert_%s_dev" % sfx, cfg._h, src, 2, n_mels, frames, 7, power, out, env=env)
            return [out.collect()]
        drive(run, PLACEMENTS, equals(want, dtype))


@row("smx_mfcc_to_mel_f32_dev", "smx_mfcc_to_mel_f64_dev")
@pytest.mark.parametrize("sfx", sorted(DTYPES))
@pytest.mark.parametrize("n_mfcc,n_mels,frames", [(13, 40, 70), (40, 40, 300), (3, 5, 1)])
def test_mfcc_to_mel(n_mfcc, n_mels, frames, sfx):
    dtype = DTYPES[sfx]
    c = (np.random.default_rng(frames).normal(size=(2, n_mfcc, frames)) * 5.0).astype(dtype)
    want = S.mfcc_to_mel(dev(c), n_mels, 22.0, 0.5).cpu().numpy()

    def run(pl):
        src, out = Region.of(c, pl[0]), Region.out(1, 2 * n_mels * frames, dtype, pl[2])
        call("smx_mfcc_to_mel_%s_dev" % sfx, src, 2, n_mfcc, frames, n_mels, 1, 22.0, 0.5, out)
        return [out.collect()]
    drive(run, PLACEMENTS, equals(want, dtype))


def test_coverage_law():
    """every device entry point of the family in the header runs in a row above (no GPU work)"""
    with open(os.path.join(ROOT, "include", "soundml_amd.h")) as fh:
        declared = set(re.findall(FAMILY, fh.read()))
    assert len(declared) == 8
    missing = sorted(declared - set(TABLE))
    assert not missing, "device entry points without a placement row: %s" % ", ".join(missing)
