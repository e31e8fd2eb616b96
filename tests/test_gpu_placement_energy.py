"""Placement of the energy device entry points: the rules of test_gpu_placement.py (guarded arena, every output word written, no
guard word touched, bit equality with the ordinary call) for the entries whose names end in `_device_f32`, which neither older
coverage law sees.  The gate is the kernel-order restatement bit for bit: a sample taken from outside a row (the arena's NaN
sentinel) or a 16-byte group assembled at the wrong offset changes bits.  This file keeps a table and a law of its own: every
name of include/soundml_amd.h matching smx_\\w+_device_f32 has a row here."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import soundml_amd as S
from soundml_amd._lib import check, lib
from conftest import ROOT
from test_gpu_placement import Region, S_OUT, S_PAD, drive, environment, host, same      # noqa: F401  (the sentinels are the arena's)

import energy_restatement as R

pytestmark = pytest.mark.gpu

TABLE = {}              # entry point -> the tests that place it
PLACEMENTS = [(0, 0, 0), (1, 0, 1), (3, 5, 3), (2, 1, 0)]       # (input offset, row pad, output offset) in elements
# the tile kernel with whole blocks and with a short last block, the general kernel; n < border
GEOMETRIES = [(2048, 512, 5000), (200, 64, 900), (16, 4, 300), (8, 11, 60), (2048, 512, 3)]
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


def bit_gate(want):
    want = np.ascontiguousarray(want, np.float32).reshape(-1)

    def gate(res, pl):
        got = host(res[0], np.float32).reshape(-1)
        differ = got.view(np.int32) != want.view(np.int32)
        assert not differ.any(), "%s: %d/%d values differ from the restatement, the first at %d" % (pl, int(differ.sum()), differ.size, int(np.argmax(differ)))
    return gate


@row("smx_rms_device_f32", "smx_zero_crossing_rate_device_f32")
@pytest.mark.parametrize("route", ["tile", "general"])
@pytest.mark.parametrize("frame_length,hop,n", GEOMETRIES)
def test_centred_faces(frame_length, hop, n, route):
    env = {"SMX_DISABLE_FAST": "1"} if route == "general" else None
    x = R.decades(n + hop, CLIPS, n, np.float32)
    count = R.frames(n, frame_length, hop)

    def rms(pl):
        xin, out = Region.of(x, pl[0], pl[1]), Region.out(1, CLIPS * count, np.float32, pl[2])
        call("smx_rms_device_f32", xin, CLIPS, n, n + pl[1], frame_length, hop, out, env=env)
        return [out.collect()]
    drive(rms, PLACEMENTS, bit_gate(R.rms_kernel_order(x, frame_length, hop)))

    def zcr(pl):
        xin, out = Region.of(x, pl[0], pl[1]), Region.out(1, CLIPS * count, np.float32, pl[2])
        call("smx_zero_crossing_rate_device_f32", xin, CLIPS, n, n + pl[1], frame_length, hop, 1e-10, out, env=env)
        return [out.collect()]
    drive(zcr, PLACEMENTS, bit_gate(R.zcr_kernel_order(x, frame_length, hop)))


@row("smx_energy_frames_device_f32")
@pytest.mark.parametrize("frame_length,hop,n", GEOMETRIES[:4])
def test_segment_face(frame_length, hop, n):
    """the stages' call: no border, so the first and the last frame end at the row's own ends, next to the sentinels"""
    x = R.decades(n, CLIPS, n, np.float32)
    count = 1 + (n - frame_length) // hop
    frames = R.segment_frames(x, frame_length, hop, count)
    for op, want in ((0, R.rms_kernel_order_of_frames(frames, hop, np.float32)), (1, R.zcr_kernel_order_of_frames(frames, hop, 0.25, np.float32))):
        def run(pl):
            xin, out = Region.of(x, pl[0], pl[1]), Region.out(1, CLIPS * count, np.float32, pl[2])
            call("smx_energy_frames_device_f32", op, 0.25, frame_length, hop, xin, CLIPS, n, n + pl[1], count, out)
            return [out.collect()]
        drive(run, PLACEMENTS, bit_gate(want))


@row("smx_rms_of_spectrogram_device_f32")
@pytest.mark.parametrize("frame_length,count", [(16, 70), (15, 300)])
def test_rms_of_spectrogram(frame_length, count):
    """a spectrogram is one packed row per call: the row pad does not apply"""
    bins = frame_length // 2 + 1
    s = np.abs(R.decades(frame_length, CLIPS * bins, count, np.float32)).reshape(CLIPS, bins, count)

    def run(pl):
        sin, out = Region.of(s, pl[0]), Region.out(1, CLIPS * count, np.float32, pl[2])
        call("smx_rms_of_spectrogram_device_f32", sin, CLIPS, bins, count, frame_length, out)
        return [out.collect()]
    drive(run, PLACEMENTS, bit_gate(R.rms_of_spectrogram_ordered(s, frame_length)))


def test_coverage_law():
    """every device entry point of the header whose name ends in _device_f32 runs in a row above (no GPU work)"""
    with open(os.path.join(ROOT, "include", "soundml_amd.h")) as fh:
        declared = set(re.findall(r"\b(smx_\w+_device_f32)\s*\(", fh.read()))
    assert len(declared) >= 4
    missing = sorted(declared - set(TABLE))
    assert not missing, "device entry points without a placement row: %s" % ", ".join(missing)
    assert not sorted(set(TABLE) - declared)
