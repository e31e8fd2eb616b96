"""Placement of the Pcen device entry points: the rules of test_gpu_placement.py (guarded arena, an offset and a row pad on the
input, offset outputs and states, every output word written, no guard word touched, bit equality with the ordinary call) for the
entries whose names match smx_pcen_\\w+_card_f32, which no older coverage law sees and which take the stream directly behind the
first argument.  The gate is the numpy restatement: a cell taken from outside a row (the arena's NaN sentinel) poisons the smoother
of that row from there on.  The tile kernel loads one element per lane from wherever a row starts: the offsets and pads put a row's
start at every 4-byte position of a 16-byte group.  This file keeps a table and a law of its own: every name of
include/soundml_amd.h matching smx_pcen_\\w+_card_f32 has a row here."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import soundml_amd as S
from soundml_amd import Mel, Pcen, Stft
from soundml_amd._lib import check, lib
from conftest import ROOT
from test_gpu_placement import Region, S_OUT, S_PAD, drive, environment, host      # noqa: F401  (the sentinels are the arena's)

import pcen_restatement as R

pytestmark = pytest.mark.gpu

TABLE = {}              # entry point -> the tests that place it
# (x offset, x row pad, output offset) in elements
PLACEMENTS = [(0, 0, 0), (1, 0, 1), (3, 5, 3), (2, 1, 0), (0, 3, 2)]
LEAD, BANDS, FRAMES = 2, 43, 2 * 64 + 37          # two row groups, the second partial; two whole tiles and a partial one
ROWS = LEAD * BANDS
ROUTES = [("tile", None), ("general", {"SMX_DISABLE_FAST": "1"})]
KW = dict(R.SETS["gain.8-bias10-power.25"], scale=2.0 ** 31)


def row(*entries):
    def mark(fn):
        for e in entries:
            TABLE.setdefault(e, []).append(fn.__name__)
        return fn
    return mark


def call(name, first, *args, env=None):
    """the first argument, the caller's stream directly behind it, then the rest"""
    import torch
    assert name in TABLE, name
    raw = [a.ptr if isinstance(a, Region) else a for a in args]
    with environment(env):
        check(getattr(lib, name)(first, C.c_void_p(torch.cuda.current_stream().cuda_stream), *raw))
        torch.cuda.synchronize()
    for a in args:
        if isinstance(a, Region) and not a.output:
            a.intact()


def gate(*wants):
    """float64 and smoothed results bit for bit; compressed float32 results (given as float64) within one float32 ulp of the
    restatement, NaN nowhere"""
    def check_all(res, pl):
        assert len(res) == len(wants)
        for k, (want, exact) in enumerate(wants):
            want = np.ascontiguousarray(want).reshape(-1)
            if exact:
                word = np.int32 if want.dtype.itemsize == 4 else np.int64
                got = host(res[k], want.dtype).reshape(-1)
                differ = got.view(word) != want.view(word)
                assert not differ.any(), "%s: result %d: %d/%d values differ from the restatement, the first at %d" % (
                    pl, k, int(differ.sum()), differ.size, int(np.argmax(differ)))
            else:
                got = host(res[k], np.float32).reshape(-1).astype(np.float64)
                near = np.abs(got - want.astype(np.float32)) <= np.spacing(np.abs(want).astype(np.float32))
                assert near.all(), "%s: result %d: %d/%d values off the restatement, the first at %d" % (
                    pl, k, int((~near).sum()), near.size, int(np.argmin(near)))
    return check_all


@row("smx_pcen_apply_card_f32")
@pytest.mark.parametrize("route", ROUTES, ids=[r[0] for r in ROUTES])
@pytest.mark.parametrize("state", [False, True], ids=["start", "zi"])
def test_apply(state, route):
    c = Pcen.Config.create(**KW)
    x = R.inputs(41, LEAD, BANDS, FRAMES)
    zi = np.ascontiguousarray(R.pcen(R.inputs(42, LEAD, BANDS, 9), **KW)[2]) if state else None
    P, _, zf = R.pcen(x, zi=zi, **KW)

    def run(pl):
        xin, out = Region.of(x, pl[0], pl[1]), Region.out(1, ROWS * FRAMES, np.float32, pl[2])
        zout = Region.out(1, ROWS, np.float64, pl[2])
        zin = Region.of(zi.reshape(-1), pl[0]) if state else None
        call("smx_pcen_apply_card_f32", c._h, xin, ROWS, FRAMES, FRAMES + pl[1], zin, out, zout, env=route[1])
        return [out.collect(), zout.collect()]
    drive(run, PLACEMENTS, gate((P, False), (zf, True)))


@row("smx_pcen_smooth_card_f32")
@pytest.mark.parametrize("route", ROUTES, ids=[r[0] for r in ROUTES])
def test_smooth(route):
    c = Pcen.Config.create(**KW)
    x = R.inputs(43, LEAD, BANDS, FRAMES)
    zi = np.ascontiguousarray(R.pcen(R.inputs(44, LEAD, BANDS, 9), **KW)[2])
    M = R.pcen(x, zi=zi, **KW)[1]

    def run(pl):
        xin, out = Region.of(x, pl[0], pl[1]), Region.out(1, ROWS * FRAMES, np.float32, pl[2])
        zin = Region.of(zi.reshape(-1), pl[0])
        call("smx_pcen_smooth_card_f32", c._h, xin, ROWS, FRAMES, FRAMES + pl[1], zin, out, env=route[1])
        return [out.collect()]
    drive(run, PLACEMENTS, gate((M.astype(np.float32), True)))


@row("smx_pcen_of_audio_card_f32")
@pytest.mark.parametrize("fft,hop", [(2048, 512), (400, 160)])
def test_of_audio(fft, hop):
    import torch
    sc = Stft.Config.create(fft_size=fft, hop=hop)
    mc = Mel.Config.create(n_mels=40, sample_rate=22050, fft_size=fft)
    c = Pcen.Config.create(hop=hop, **KW)
    n = hop * 70 + 17
    x = np.random.default_rng(45).uniform(-1, 1, size=(3, n)).astype(np.float32)
    frames = Stft.frames(sc, n)
    # the composition on the restatement: the mel spectrogram the library computes, then the numpy smoother and compression
    mel = S.mel_spectrogram(sc, mc, torch.from_numpy(x).cuda(), power=1.0).cpu().numpy()
    want = R.pcen(mel, hop=hop, **KW)[0]

    def run(pl):
        xin, out = Region.of(x, pl[0], pl[1]), Region.out(1, 3 * 40 * frames, np.float32, pl[2])
        call("smx_pcen_of_audio_card_f32", c._h, sc._h, mc._h, xin, 3, n, n + pl[1], out)
        return [out.collect()]
    drive(run, PLACEMENTS, gate((want, False)))


@row("smx_pcen_kernel_step_card_f32")
@pytest.mark.parametrize("route", ROUTES, ids=[r[0] for r in ROUTES])
def test_kernel_step(route):
    """three chunks, each from and into its own placed buffers: a few frames (the general kernel), whole tiles and more, a tail"""
    c = Pcen.Config.create(**KW)
    x = R.inputs(46, LEAD, BANDS, FRAMES)
    P = R.pcen(x, **KW)[0]
    cuts = [0, 5, 64 + 41, FRAMES]
    k = Pcen.Kernel.prepare(c, LEAD, BANDS)

    def run(pl):
        k.reset()
        res = []
        for a, b in zip(cuts[:-1], cuts[1:]):
            xin, out = Region.of(np.ascontiguousarray(x[..., a:b]), pl[0], pl[1]), Region.out(1, ROWS * (b - a), np.float32, pl[2])
            call("smx_pcen_kernel_step_card_f32", k._h, xin, b - a, b - a + pl[1], out, env=route[1])
            res.append(out.collect())
        return res
    drive(run, PLACEMENTS, gate(*[(P[..., a:b], False) for a, b in zip(cuts[:-1], cuts[1:])]))


def test_coverage_law():
    """every device entry point of the header whose name matches smx_pcen_\\w+_card_f32 runs in a row above (no GPU work)"""
    with open(os.path.join(ROOT, "include", "soundml_amd.h")) as fh:
        declared = set(re.findall(r"\b(smx_pcen_\w+_card_f32)\s*\(", fh.read()))
    assert len(declared) >= 4
    missing = sorted(declared - set(TABLE))
    assert not missing, "device entry points without a placement row: %s" % ", ".join(missing)
    assert not sorted(set(TABLE) - declared)
