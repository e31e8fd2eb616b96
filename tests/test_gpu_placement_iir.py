"""Placement of the Iir device entry points: the rules of test_gpu_placement.py (guarded arena, an offset and a row pad on the
input, offset outputs, every output word written, no guard word touched, bit equality with the ordinary call) for the entries
whose names end in `_card_f32`, which no older coverage law sees and which take the stream directly behind the handle.  The gate
is the numpy restatement: a sample taken from outside a row (the arena's NaN sentinel) poisons the recursion from there on.  The
block route stages a wave's span in coalesced loads from wherever the row starts: the offsets put a row's start at every 4-byte
position of a 16-byte group.  This file keeps a table and a law of its own: every name of include/soundml_amd.h matching
smx_iir_\\w+_card_f32 has a row here."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from soundml_amd import Iir
from soundml_amd._lib import check, lib
from conftest import ROOT
from test_gpu_placement import Region, S_OUT, S_PAD, drive, environment, host      # noqa: F401  (the sentinels are the arena's)

import iir_restatement as R

pytestmark = pytest.mark.gpu

TABLE = {}              # entry point -> the tests that place it
# (x offset, x row pad, output offset) in elements
PLACEMENTS = [(0, 0, 0), (1, 0, 1), (3, 5, 3), (2, 1, 0), (0, 3, 2)]
B = Iir.BLOCK
LEAD, N = 3, 2 * B + 37          # two whole blocks through the block route and a tail through the general kernel
ROUTES = [("block", None), ("general", {"SMX_DISABLE_FAST": "1"})]
SECTIONS = [2, 5]


def row(*entries):
    def mark(fn):
        for e in entries:
            TABLE.setdefault(e, []).append(fn.__name__)
        return fn
    return mark


def call(name, handle, *args, env=None):
    """the handle, the caller's stream directly behind it, then the rest"""
    import torch
    assert name in TABLE, name
    raw = [a.ptr if isinstance(a, Region) else a for a in args]
    with environment(env):
        check(getattr(lib, name)(handle, C.c_void_p(torch.cuda.current_stream().cuda_stream), *raw))
        torch.cuda.synchronize()
    for a in args:
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


@row("smx_iir_apply_card_f32")
@pytest.mark.parametrize("route", ROUTES, ids=[r[0] for r in ROUTES])
@pytest.mark.parametrize("s", SECTIONS)
def test_apply(s, route):
    c = Iir.Config.create(R.cascade(s))
    x = R.batch(31, LEAD, N)
    for kind in (None, "call", "rows"):
        want, zf = R.expected(s, 31, LEAD, N, kind)
        zi = None if kind is None else np.ascontiguousarray(R.batch_state(32, 1, s)[0] if kind == "call" else R.batch_state(32, LEAD, s))

        def run(pl):
            xin, out = Region.of(x, pl[0], pl[1]), Region.out(1, LEAD * N, np.float32, pl[2])
            state = Region.out(1, LEAD * 2 * s, np.float64, pl[2])
            rows = Region.of(zi.reshape(-1), pl[0]) if kind == "rows" else None
            call("smx_iir_apply_card_f32", c._h, xin, LEAD, N, N + pl[1], C.c_void_p(zi.ctypes.data) if kind == "call" else None,
                 rows if kind == "rows" else None, out, state, env=route[1])
            return [out.collect(), state.collect()]
        drive(run, PLACEMENTS, bit_gate(want.astype(np.float32), zf))


@row("smx_iir_filtfilt_card_f32")
@pytest.mark.parametrize("route", ROUTES, ids=[r[0] for r in ROUTES])
@pytest.mark.parametrize("s", SECTIONS)
def test_filtfilt(s, route):
    c = Iir.Config.create(R.cascade(s))
    x = R.batch(33, LEAD, N)
    want = R.expected_filtfilt(s, 33, LEAD, N)

    def run(pl):
        xin, out = Region.of(x, pl[0], pl[1]), Region.out(1, LEAD * N, np.float32, pl[2])
        call("smx_iir_filtfilt_card_f32", c._h, xin, LEAD, N, N + pl[1], out, env=route[1])
        return [out.collect()]
    drive(run, PLACEMENTS, bit_gate(want.astype(np.float32)))


@row("smx_iir_kernel_step_card_f32")
@pytest.mark.parametrize("route", ROUTES, ids=[r[0] for r in ROUTES])
@pytest.mark.parametrize("s", SECTIONS)
def test_kernel_step(s, route):
    """three chunks, each from and into its own placed buffers: a head inside a block, whole blocks, a tail"""
    c = Iir.Config.create(R.cascade(s))
    x = R.batch(34, LEAD, N)
    want = R.expected(s, 34, LEAD, N)[0].astype(np.float32)
    cuts = [0, 41, B + 90, N]
    k = Iir.Kernel.prepare(c, LEAD)

    def run(pl):
        k.reset()
        res = []
        for a, b in zip(cuts[:-1], cuts[1:]):
            xin, out = Region.of(np.ascontiguousarray(x[:, a:b]), pl[0], pl[1]), Region.out(1, LEAD * (b - a), np.float32, pl[2])
            call("smx_iir_kernel_step_card_f32", k._h, xin, b - a, b - a + pl[1], out, env=route[1])
            res.append(out.collect())
        return res
    drive(run, PLACEMENTS, bit_gate(*[want[:, a:b] for a, b in zip(cuts[:-1], cuts[1:])]))


def test_coverage_law():
    """every device entry point of the header whose name ends in _card_f32 runs in a row above (no GPU work)"""
    with open(os.path.join(ROOT, "include", "soundml_amd.h")) as fh:
        declared = set(re.findall(r"\b(smx_iir_\w+_card_f32)\s*\(", fh.read()))
    assert len(declared) >= 3
    missing = sorted(declared - set(TABLE))
    assert not missing, "device entry points without a placement row: %s" % ", ".join(missing)
    assert not sorted(set(TABLE) - declared)
