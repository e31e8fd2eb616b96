"""Placement of the pYIN device entry points: the rules of test_gpu_placement.py (guarded arena, every output word written, no guard
word touched, bit equality with the ordinary call) for the entries whose names end in `_accel_f32`, which no older coverage law
sees.  The gate is the numpy restatement bit for bit: a sample or an observation taken from outside a row (the arena's NaN sentinel)
changes bits.  This file keeps a table and a law of its own: every name of include/soundml_amd.h matching smx_\\w+_accel_f32 has a
row here."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import soundml_amd as S
from soundml_amd import Pitch
from soundml_amd._lib import check, lib
from conftest import ROOT
from test_gpu_placement import Region, S_OUT, S_PAD, drive, environment, host, same      # noqa: F401  (the sentinels are the arena's)
from test_gpu_placement_pitch import bit_gate

import pitch_restatement as P
import pyin_restatement as R

pytestmark = pytest.mark.gpu

TABLE = {}              # entry point -> the tests that place it
PLACEMENTS = [(0, 0, 0), (1, 0, 1), (3, 5, 3), (2, 1, 0)]       # (input offset, row pad, output offset) in elements
# 602 bins with 16-bit pointers on the tile route; 39 bins with the band wider than the state axis, 8-bit pointers; the general route
GEOMETRIES = [(2048, 512, 5000, 22050, 65.0, 2093.0), (256, 64, 1500, 8000, 400.0, 500.0), (33, 7, 90, 8000, 600.0, 3000.0)]
CLIPS = 2
DEFAULTS = (100, 2.0, 18.0, 2.0, 0.1, 35.92, 0.01, 0.01)


def row(*entries):
    def mark(fn):
        for e in entries:
            TABLE.setdefault(e, []).append(fn.__name__)
        return fn
    return mark


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


@row("smx_pyin_accel_f32", "smx_pyin_observation_accel_f32")
@pytest.mark.parametrize("frame_length,hop,n,sr,fmin,fmax", GEOMETRIES)
def test_audio_faces(frame_length, hop, n, sr, fmin, fmax):
    x = P.decades(n + hop, CLIPS, n, np.float32)
    tab = Pitch.pyin_tables(fmin, fmax, sample_rate=sr, frame_length=frame_length, hop=hop)
    count, states = R.frames(n, frame_length, hop), 2 * tab["n_bins"]
    f0, flag, prob = R.pyin(x, fmin, fmax, tab, sr, frame_length, hop, fill_na=None)
    params = (sr, fmin, fmax, frame_length, hop) + DEFAULTS

    def pyin(pl):
        xin = Region.of(x, pl[0], pl[1])
        outs = [Region.out(1, CLIPS * count, np.float32, pl[2]) for _ in range(3)]
        call("smx_pyin_accel_f32", xin, CLIPS, n, n + pl[1], *params, 1, 0.0, *outs)
        return [o.collect() for o in outs]
    drive(pyin, PLACEMENTS, bit_gate(f0, flag, prob))

    def observation(pl):
        xin, out = Region.of(x, pl[0], pl[1]), Region.out(1, CLIPS * states * count, np.float32, pl[2])
        call("smx_pyin_observation_accel_f32", xin, CLIPS, n, n + pl[1], *params, out)
        return [out.collect()]
    drive(observation, PLACEMENTS, bit_gate(R.pyin_observation(x, fmin, fmax, tab, sr, frame_length, hop)))


@row("smx_pyin_decode_accel_f32")
@pytest.mark.parametrize("nb,h,T", [(61, 10, 40), (17, 70, 9), (40, 0, 5), (23, 3, 1)])
def test_decode_face(nb, h, T):
    """clips clip_stride apart: the last state's row of a clip ends next to the sentinels"""
    rng = np.random.default_rng(nb + h)
    obs = rng.uniform(0.0, 1.0, (CLIPS, 2 * nb, T)).astype(np.float32)
    obs[:, :nb] *= rng.uniform(0.0, 1.0, (CLIPS, nb, T)) < 0.1            # sparse voiced candidates
    tri = 1.0 - np.abs(np.arange(2 * h + 1) - h) / float(h + 1)
    rs = np.array([1.0 / sum([tri[j - i + h] for j in range(max(0, i - h), min(nb - 1, i + h) + 1)]) for i in range(nb)])
    want = R.pyin_decode(obs, tri, rs, 0.05)

    def run(pl):
        oin, out = Region.of(obs.reshape(CLIPS, -1), pl[0], pl[1]), Region.out(1, CLIPS * T, np.float32, pl[2])
        call("smx_pyin_decode_accel_f32", oin, CLIPS, 2 * nb, T, 2 * nb * T + pl[1], h, 0.05, out)
        return [out.collect()]
    drive(run, PLACEMENTS, bit_gate(want))


def test_coverage_law():
    """every device entry point of the header whose name ends in _accel_f32 runs in a row above (no GPU work)"""
    with open(os.path.join(ROOT, "include", "soundml_amd.h")) as fh:
        declared = set(re.findall(r"\b(smx_\w+_accel_f32)\s*\(", fh.read()))
    assert len(declared) >= 3
    missing = sorted(declared - set(TABLE))
    assert not missing, "device entry points without a placement row: %s" % ", ".join(missing)
    assert not sorted(set(TABLE) - declared)
