"""Placement of the Pitch device entry points: the rules of test_gpu_placement.py (guarded arena, every output word written, no
guard word touched, bit equality with the ordinary call) for the entries whose names end in `_resident_f32`, which no older
coverage law sees.  The gate is the numpy restatement bit for bit: a sample taken from outside a row (the arena's NaN sentinel) or
a 16-byte group assembled at the wrong offset changes bits.  This file keeps a table and a law of its own: every name of
include/soundml_amd.h matching smx_\\w+_resident_f32 has a row here."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import soundml_amd as S
from soundml_amd._lib import check, lib
from conftest import ROOT
from test_gpu_placement import Region, S_OUT, S_PAD, drive, environment, host, same      # noqa: F401  (the sentinels are the arena's)

import pitch_restatement as R

pytestmark = pytest.mark.gpu

TABLE = {}              # entry point -> the tests that place it
PLACEMENTS = [(0, 0, 0), (1, 0, 1), (3, 5, 3), (2, 1, 0)]       # (input offset, row pad, output offset) in elements
# the tile route with whole blocks and with a short last block, the general route; n < border
GEOMETRIES = [(2048, 512, 5000, 22050, 65.0, 2093.0), (200, 64, 900, 8000, 100.0, 1000.0), (64, 16, 300, 8000, 300.0, 2000.0),
              (33, 7, 90, 8000, 600.0, 3000.0), (2048, 512, 3, 22050, 65.0, 2093.0)]
CLIPS = 2


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


@row("smx_yin_resident_f32", "smx_yin_difference_resident_f32")
@pytest.mark.parametrize("route", ["tile", "general"])
@pytest.mark.parametrize("frame_length,hop,n,sr,fmin,fmax", GEOMETRIES)
def test_centred_faces(frame_length, hop, n, sr, fmin, fmax, route):
    env = {"SMX_DISABLE_FAST": "1"} if route == "general" else None
    x = R.decades(n + hop, CLIPS, n, np.float32)
    count, lags = R.frames(n, frame_length, hop), R.lag_range(sr, fmin, fmax, frame_length)[1] + 1
    f0, ap = R.yin(x, fmin, fmax, sr, frame_length, hop)

    def yin(pl):
        xin = Region.of(x, pl[0], pl[1])
        o0, o1 = Region.out(1, CLIPS * count, np.float32, pl[2]), Region.out(1, CLIPS * count, np.float32, pl[2])
        call("smx_yin_resident_f32", xin, CLIPS, n, n + pl[1], sr, fmin, fmax, frame_length, hop, 0.1, o0, o1, env=env)
        return [o0.collect(), o1.collect()]
    drive(yin, PLACEMENTS, bit_gate(f0, ap))

    def alone(pl):
        xin, o0 = Region.of(x, pl[0], pl[1]), Region.out(1, CLIPS * count, np.float32, pl[2])
        call("smx_yin_resident_f32", xin, CLIPS, n, n + pl[1], sr, fmin, fmax, frame_length, hop, 0.1, o0, None, env=env)
        return [o0.collect()]
    drive(alone, PLACEMENTS[:2], bit_gate(f0))

    def difference(pl):
        xin, out = Region.of(x, pl[0], pl[1]), Region.out(1, CLIPS * lags * count, np.float32, pl[2])
        call("smx_yin_difference_resident_f32", xin, CLIPS, n, n + pl[1], sr, fmin, fmax, frame_length, hop, out, env=env)
        return [out.collect()]
    drive(difference, PLACEMENTS, bit_gate(R.yin_difference(x, fmin, fmax, sr, frame_length, hop)))


@row("smx_yin_frames_resident_f32")
@pytest.mark.parametrize("frame_length,hop,n,sr,fmin,fmax", GEOMETRIES[:4])
def test_segment_face(frame_length, hop, n, sr, fmin, fmax):
    """the stage's call: no border, so the first and the last frame end at the row's own ends, next to the sentinels"""
    x = R.decades(n, CLIPS, n, np.float32)
    count = 1 + (n - frame_length) // hop
    index = np.arange(count)[:, None] * hop + np.arange(frame_length)[None, :]
    f0, ap = R.yin_of_frames(x[..., index].astype(np.float64), hop, sr, fmin, fmax, 0.1, np.float32)

    def run(pl):
        xin = Region.of(x, pl[0], pl[1])
        o0, o1 = Region.out(1, CLIPS * count, np.float32, pl[2]), Region.out(1, CLIPS * count, np.float32, pl[2])
        call("smx_yin_frames_resident_f32", xin, CLIPS, n, n + pl[1], count, sr, fmin, fmax, frame_length, hop, 0.1, o0, o1)
        return [o0.collect(), o1.collect()]
    drive(run, PLACEMENTS, bit_gate(f0, ap))


def test_coverage_law():
    """every device entry point of the header whose name ends in _resident_f32 runs in a row above (no GPU work)"""
    with open(os.path.join(ROOT, "include", "soundml_amd.h")) as fh:
        declared = set(re.findall(r"\b(smx_\w+_resident_f32)\s*\(", fh.read()))
    assert len(declared) >= 3
    missing = sorted(declared - set(TABLE))
    assert not missing, "device entry points without a placement row: %s" % ", ".join(missing)
    assert not sorted(set(TABLE) - declared)
