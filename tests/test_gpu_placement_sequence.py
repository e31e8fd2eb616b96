"""Placement of the Sequence device entry points: the rules of test_gpu_placement.py (guarded arena, offsets and row pads on both
inputs, an offset output, every output word written, no guard word touched, bit equality with the ordinary call) for the entries
whose names end in `_hbm_f32`, which no older coverage law sees.  The gate is the numpy restatement: a value taken from outside a
row (the arena's NaN sentinel) changes the cost's bits, and with them D, the path and the distance.  The cost kernel fetches whole
aligned 16-byte groups around a row: the offsets put a row's start at every position of such a group.  This file keeps a table and
a law of its own: every name of include/soundml_amd.h matching smx_\\w+_hbm_f32 has a row here."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import soundml_amd as S
from soundml_amd import Sequence
from soundml_amd._lib import METRIC, check, lib
from conftest import ROOT
from test_gpu_placement import Region, S_OUT, S_PAD, drive, environment, host, same      # noqa: F401  (the sentinels are the arena's)

import sequence_restatement as R

pytestmark = pytest.mark.gpu

TABLE = {}              # entry point -> the tests that place it
# (X offset, X row pad, Y offset, Y row pad, output offset) in elements
PLACEMENTS = [(0, 0, 0, 0, 0), (1, 0, 2, 0, 1), (3, 5, 1, 3, 3), (2, 1, 3, 2, 0), (0, 3, 0, 1, 2)]
TR, TC = Sequence.TILE_ROWS, Sequence.TILE_COLS
# two by two tiles with short last ones; n < 64 over two tile columns
GEOMETRIES = [(5, TR + 3, TC + 7), (3, 37, TC + 2)]
PAIRS = 3
ZEROS, ONES = (C.c_double * 3)(0, 0, 0), (C.c_double * 3)(1, 1, 1)
SKEWED = (C.c_double * 3)(0, 0.5, 0.25), (C.c_double * 3)(2, 1, 1)


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


ROUTES = [("tile", None), ("general", {"SMX_DISABLE_FAST": "1"})]


@row("smx_cost_matrix_hbm_f32")
@pytest.mark.parametrize("route", ROUTES, ids=[r[0] for r in ROUTES])
@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_cost_matrix(geometry, route):
    d, n, m = geometry
    x, y = R.pair_batch(geometry)
    for metric in ("euclidean", "cosine"):
        want = R.cost_matrix(x, y, metric)

        def run(pl):
            xin, yin, out = Region.of(x, pl[0], pl[1]), Region.of(y, pl[2], pl[3]), Region.out(1, PAIRS * n * m, np.float32, pl[4])
            call("smx_cost_matrix_hbm_f32", xin, yin, PAIRS, d, n, m, n + pl[1], m + pl[3], METRIC[metric], out, env=route[1])
            return [out.collect()]
        drive(run, PLACEMENTS, bit_gate(want))


@row("smx_dtw_hbm_f32", "smx_dtw_distance_hbm_f32")
@pytest.mark.parametrize("route", ROUTES, ids=[r[0] for r in ROUTES])
@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_dtw_and_distance(geometry, route):
    d, n, m = geometry
    x, y = R.pair_batch(geometry)
    for subseq, (add, mul) in ((0, (ZEROS, ONES)), (1, SKEWED)):
        D, path, dist = R.dtw(x, y, "euclidean", list(add), list(mul), bool(subseq))

        def run(pl):
            xin, yin = Region.of(x, pl[0], pl[1]), Region.of(y, pl[2], pl[3])
            o0, o1 = Region.out(1, PAIRS * n * m, np.float32, pl[4]), Region.out(1, PAIRS * 2 * (n + m - 1), np.float32, pl[4])
            call("smx_dtw_hbm_f32", xin, yin, PAIRS, d, n, m, n + pl[1], m + pl[3], METRIC["euclidean"], add, mul, subseq, o0, o1, env=route[1])
            return [o0.collect(), o1.collect()]
        drive(run, PLACEMENTS, bit_gate(D, path))

        def distance(pl):
            xin, yin, out = Region.of(x, pl[0], pl[1]), Region.of(y, pl[2], pl[3]), Region.out(1, PAIRS, np.float32, pl[4])
            call("smx_dtw_distance_hbm_f32", xin, yin, PAIRS, d, n, m, n + pl[1], m + pl[3], METRIC["euclidean"], add, mul, subseq, out, env=route[1])
            return [out.collect()]
        drive(distance, PLACEMENTS, bit_gate(dist))


def test_coverage_law():
    """every device entry point of the header whose name ends in _hbm_f32 runs in a row above (no GPU work)"""
    with open(os.path.join(ROOT, "include", "soundml_amd.h")) as fh:
        declared = set(re.findall(r"\b(smx_\w+_hbm_f32)\s*\(", fh.read()))
    assert len(declared) >= 3
    missing = sorted(declared - set(TABLE))
    assert not missing, "device entry points without a placement row: %s" % ", ".join(missing)
    assert not sorted(set(TABLE) - declared)
