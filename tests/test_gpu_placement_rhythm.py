"""Placement of the Rhythm device entry points: the rules of test_gpu_placement.py (guarded arena, every output word written, no
guard word touched, bit equality with the ordinary call) for the entries whose names end in `_gpu_f32`, which no older coverage
law sees.  The gate is the numpy restatement: a value taken from outside a row (the arena's NaN sentinel) changes the tempogram's
bits, the lag and the beats.  This file keeps a table and a law of its own: every name of include/soundml_amd.h matching
smx_\\w+_gpu_f32 has a row here."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import soundml_amd as S
from soundml_amd import Rhythm, Window
from soundml_amd._lib import WINDOW, check, lib
from conftest import ROOT
from test_gpu_placement import Region, S_OUT, S_PAD, drive, environment, host, same      # noqa: F401  (the sentinels are the arena's)

import rhythm_restatement as R

pytestmark = pytest.mark.gpu

TABLE = {}              # entry point -> the tests that place it
PLACEMENTS = [(0, 0, 0), (1, 0, 1), (3, 5, 3), (2, 1, 0)]       # (input offset, row pad, output offset) in elements
# two tiles of frames with a short second one; an odd window; frames < window
GEOMETRIES = [R.GEOMETRIES[0], R.GEOMETRIES[3], R.GEOMETRIES[4]]
CLIPS = 3


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


def call(name, *args, env=None):
    import torch
    assert name in TABLE, name
    raw = [a.ptr if isinstance(a, Region) else a for a in args]
    with environment(env):
        check(getattr(lib, name)(*raw, C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        torch.cuda.synchronize()
    for a in args:
        if isinstance(a, Region) and not a.output:
            a.intact()


def bit_gate(*wants):
    wants = [np.ascontiguousarray(w, np.float32).reshape(-1) for w in wants]

    def gate(res, pl):
        assert len(res) == len(wants)
        for k, want in enumerate(wants):
            got = host(res[k], np.float32).reshape(-1)
            differ = got.view(np.int32) != want.view(np.int32)
            assert not differ.any(), "%s: result %d: %d/%d values differ from the restatement, the first at %d" % (
                pl, k, int(differ.sum()), differ.size, int(np.argmax(differ)))
    return gate


@row("smx_rhythm_tempogram_gpu_f32")
@pytest.mark.parametrize("route", ["tile", "general"])
@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_tempogram(geometry, route):
    frames, p, W = geometry[:3]
    env = {"SMX_DISABLE_FAST": "1"} if route == "general" else None
    x = R.click_batch(geometry)
    for norm in (1, 0):
        want = R.tempogram(x, Window.make(np.float64, "hann", W), bool(norm))

        def run(pl):
            xin, out = Region.of(x, pl[0], pl[1]), Region.out(1, CLIPS * W * frames, np.float32, pl[2])
            call("smx_rhythm_tempogram_gpu_f32", xin, CLIPS, frames, frames + pl[1], W, WINDOW["hann"], 0.0, norm, out, env=env)
            return [out.collect()]
        drive(run, PLACEMENTS, bit_gate(want))


@row("smx_rhythm_tempo_gpu_f32", "smx_rhythm_beat_track_gpu_f32")
@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_tempo_and_beat_track(geometry):
    frames, p, W, sr, hop = geometry
    x = R.click_batch(geometry)
    lags, gaps = R.tempo_lag(x, Window.make(np.float64, "hann", W), Rhythm.tempo_prior(W, sr, hop))
    assert np.all(gaps > 1e-6)
    freq = Rhythm.tempo_frequencies(W, sr, hop)

    def masks(periods):
        rows = []
        for c in range(CLIPS):
            g, tx = Rhythm.beat_tables(int(periods[c]))
            rows.append(R.mask_of(R.beats_of(x[c], int(periods[c]), g, tx, True), frames, np.float32))
        return np.stack(rows)

    for want_lag, want in ((1, lags.astype(np.float32)), (0, freq[lags].astype(np.float32))):
        def tempo(pl):
            xin, out = Region.of(x, pl[0], pl[1]), Region.out(1, CLIPS, np.float32, pl[2])
            call("smx_rhythm_tempo_gpu_f32", xin, CLIPS, frames, frames + pl[1], sr, hop, W, 120.0, 1.0, 320.0, want_lag, out)
            return [out.collect()]
        drive(tempo, PLACEMENTS, bit_gate(want))

    given = float(freq[p])
    for has, bpm, tempi, beats in ((0, 0.0, freq[lags], masks(lags)), (1, given, np.full(CLIPS, given), masks([p] * CLIPS))):
        def track(pl):
            xin = Region.of(x, pl[0], pl[1])
            o0, o1 = Region.out(1, CLIPS, np.float32, pl[2]), Region.out(1, CLIPS * frames, np.float32, pl[2])
            call("smx_rhythm_beat_track_gpu_f32", xin, CLIPS, frames, frames + pl[1], sr, hop, has, bpm, W, 120.0, 100.0, 1, o0, o1)
            return [o0.collect(), o1.collect()]
        drive(track, PLACEMENTS, bit_gate(tempi.astype(np.float32), beats))


def test_coverage_law():
    """every device entry point of the header whose name ends in _gpu_f32 runs in a row above (no GPU work)"""
    with open(os.path.join(ROOT, "include", "soundml_amd.h")) as fh:
        declared = set(re.findall(r"\b(smx_\w+_gpu_f32)\s*\(", fh.read()))
    assert len(declared) >= 3
    missing = sorted(declared - set(TABLE))
    assert not missing, "device entry points without a placement row: %s" % ", ".join(missing)
    assert not sorted(set(TABLE) - declared)
