"""Placement of the Loudness device entry points: the rules of test_gpu_placement.py (guarded arena, an offset and a row pad on the
input, offset outputs, every output word written, no guard word touched, bit equality with the ordinary call) for the entries
whose names match smx_loudness_\\w+_card_f32, which no older coverage law sees and which take the stream directly behind the first
argument.  The gate is the numpy restatement: a sample taken from outside a row (the arena's NaN sentinel) poisons the energies
and the peak.  True peak reads its rows in aligned 16-byte loads from wherever a row starts: the offsets and pads put a row's
start at every 4-byte position of a 16-byte group.  This file keeps a table and a law of its own: every name of
include/soundml_amd.h matching smx_loudness_\\w+_card_f32 has a row here."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from soundml_amd import Iir, Loudness
from soundml_amd._lib import check, lib
from conftest import ROOT
from test_gpu_placement import Region, S_OUT, S_PAD, drive, environment, host      # noqa: F401  (the sentinels are the arena's)

import loudness_restatement as R

pytestmark = pytest.mark.gpu

TABLE = {}              # entry point -> the tests that place it
# (x offset, x row pad, output offset) in elements
PLACEMENTS = [(0, 0, 0), (1, 0, 1), (3, 5, 3), (2, 1, 0), (0, 3, 2)]
B = Iir.BLOCK
RATE = 8000
STEP = R.step(RATE)
CLIPS, CHANNELS, N = 2, 2, 30 * STEP + 2 * B + 37      # 27 blocks, one short-term window; whole Iir blocks and a tail
ROUTES = [("block", None), ("general", {"SMX_DISABLE_FAST": "1"})]
WEIGHTS = np.array([1.0, 0.5])
WP = C.c_void_p(WEIGHTS.ctypes.data)


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
    raw = [a.ptr if isinstance(a, Region) else a for a in (first,) + args]
    with environment(env):
        check(getattr(lib, name)(raw[0], C.c_void_p(torch.cuda.current_stream().cuda_stream), *raw[1:]))
        torch.cuda.synchronize()
    for a in (first,) + args:
        if isinstance(a, Region) and not a.output:
            a.intact()


def bit_gate(*wants):
    wants = [np.ascontiguousarray(w).reshape(-1) for w in wants]

    def gate(res, pl):
        assert len(res) == len(wants)
        for k, want in enumerate(wants):
            word = np.int32 if want.dtype.itemsize == 4 else np.int64
            got = host(res[k], want.dtype).reshape(-1)
            differ = got.view(word) != want.view(word)
            assert not differ.any(), "%s: result %d: %d/%d values differ from the restatement, the first at %d" % (
                pl, k, int(differ.sum()), differ.size, int(np.argmax(differ)))
    return gate


def ulp_gate(*wants):
    """float32 results within one float32 ulp of the restatement's float64 (the device's log10 and pow are not numpy's)"""
    wants = [np.ascontiguousarray(w, dtype=np.float64).reshape(-1) for w in wants]

    def gate(res, pl):
        assert len(res) == len(wants)
        for k, want in enumerate(wants):
            got = host(res[k], np.float32).reshape(-1).astype(np.float64)
            live = np.isfinite(want)
            assert np.array_equal(got[~live], want[~live]), (pl, k)
            assert np.all(np.abs(got[live] - want[live]) <= np.spacing(np.abs(want[live]).astype(np.float32))), (pl, k)
    return gate


def audio(seed=51):
    return np.array(R.noise(seed, CLIPS, CHANNELS, N)) * np.array([1.0, 0.05], np.float32)[:, None, None]


def placed(x, pl):
    return Region.of(x, pl[0], pl[1])


@row("smx_loudness_block_energy_card_f32")
@pytest.mark.parametrize("route", ROUTES, ids=[r[0] for r in ROUTES])
def test_block_energy(route):
    x = audio()
    m = R.measure(x, RATE)
    nb = R.blocks(RATE, N)

    def run(pl):
        out = Region.out(1, CLIPS * CHANNELS * nb, np.float64, pl[2])
        call("smx_loudness_block_energy_card_f32", placed(x, pl), CLIPS, CHANNELS, N, N + pl[1], RATE, out, env=route[1])
        return [out.collect()]
    drive(run, PLACEMENTS, bit_gate(m.z))


@row("smx_loudness_momentary_card_f32")
@pytest.mark.parametrize("short_term", [0, 1])
def test_momentary(short_term):
    x = audio()
    m = R.measure(x, RATE, WEIGHTS)
    want = m.short_term if short_term else m.momentary

    def run(pl):
        out = Region.out(1, want.size, np.float32, pl[2])
        call("smx_loudness_momentary_card_f32", placed(x, pl), CLIPS, CHANNELS, N, N + pl[1], RATE, WP, short_term, out)
        return [out.collect()]
    drive(run, PLACEMENTS, ulp_gate(want))


@row("smx_loudness_integrated_card_f32")
@pytest.mark.parametrize("route", ROUTES, ids=[r[0] for r in ROUTES])
def test_integrated(route):
    x = audio()
    m = R.measure(x, RATE, WEIGHTS)

    def run(pl):
        out = Region.out(1, CLIPS, np.float32, pl[2])
        call("smx_loudness_integrated_card_f32", placed(x, pl), CLIPS, CHANNELS, N, N + pl[1], RATE, WP, out, None, env=route[1])
        return [out.collect()]
    drive(run, PLACEMENTS, ulp_gate(m.integrated))


@row("smx_loudness_true_peak_card_f32")
@pytest.mark.parametrize("n", [13, 4 * 1024 + 3])
def test_true_peak(n):
    x = np.ascontiguousarray(audio()[..., :n])
    want = R.true_peak(x.reshape(-1, n), Loudness.true_peak_taps()).astype(np.float32)

    def run(pl):
        out = Region.out(1, CLIPS * CHANNELS, np.float32, pl[2])
        call("smx_loudness_true_peak_card_f32", placed(x, pl), CLIPS * CHANNELS, n, n + pl[1], out)
        return [out.collect()]
    drive(run, PLACEMENTS, bit_gate(want))


@row("smx_loudness_normalize_card_f32")
@pytest.mark.parametrize("ceiling", [None, 0.1])
def test_normalize(ceiling):
    x = audio()
    m = R.measure(x, RATE, WEIGHTS)
    peaks = R.true_peak(x.reshape(-1, N), Loudness.true_peak_taps()).reshape(CLIPS, CHANNELS)
    gains = np.array([R.gain(m.integrated[c], peaks[c], -23.0, ceiling) for c in range(CLIPS)])

    def run(pl):
        out = Region.out(1, x.size, np.float32, pl[2])
        call("smx_loudness_normalize_card_f32", placed(x, pl), CLIPS, CHANNELS, N, N + pl[1], RATE, -23.0, 0 if ceiling is None else 1, ceiling or 0.0, WP, out)
        return [out.collect()]
    drive(run, PLACEMENTS, ulp_gate(gains[:, None, None] * x.astype(np.float64)))


@row("smx_loudness_meter_step_card_f32", "smx_loudness_meter_read_card_f32")
@pytest.mark.parametrize("route", ROUTES, ids=[r[0] for r in ROUTES])
def test_meter(route):
    """three chunks, each from its own placed buffer into placed results: a head inside a block, whole blocks, a tail; then both reads"""
    x = audio()
    m = R.measure(x, RATE, WEIGHTS)
    cuts = [0, 41, 28 * STEP + 90, N]
    done = [max(0, c // STEP - 3) for c in cuts]
    k = Loudness.Meter.prepare(RATE, CLIPS, CHANNELS, weights=WEIGHTS)

    def run(pl):
        k.reset()
        res = []
        for (a, b), (ja, jb) in zip(zip(cuts[:-1], cuts[1:]), zip(done[:-1], done[1:])):
            xin = Region.of(np.ascontiguousarray(x[..., a:b]), pl[0], pl[1])
            out = Region.out(1, CLIPS * (jb - ja), np.float32, pl[2]) if jb > ja else None
            call("smx_loudness_meter_step_card_f32", k._h, xin, b - a, b - a + pl[1], out, env=route[1])
            if out is not None:
                res.append(out.collect())
        for what, count in ((0, 1), (1, done[-1] - 26)):
            out = Region.out(1, CLIPS * count, np.float32, pl[2])
            call("smx_loudness_meter_read_card_f32", k._h, what, out, env=route[1])
            res.append(out.collect())
        return res
    wants = [m.momentary[:, ja:jb] for ja, jb in zip(done[:-1], done[1:]) if jb > ja] + [m.integrated, m.short_term]
    drive(run, PLACEMENTS, ulp_gate(*wants))


def test_coverage_law():
    """every device entry point of the header whose name matches smx_loudness_\\w+_card_f32 runs in a row above (no GPU work)"""
    with open(os.path.join(ROOT, "include", "soundml_amd.h")) as fh:
        declared = set(re.findall(r"\b(smx_loudness_\w+_card_f32)\s*\(", fh.read()))
    assert len(declared) >= 7
    missing = sorted(declared - set(TABLE))
    assert not missing, "device entry points without a placement row: %s" % ", ".join(missing)
    assert not sorted(set(TABLE) - declared)
