"""Streams: the Iir device entry points on a held side stream, by the method of test_gpu_streams.py (the decoy inputs, the hold,
the true inputs copied in behind it, `pending` read at once, the bits after the wait, a warm call back within H / 2).  Those
entries end in `_card_f32` and take the stream directly behind the handle, so test_gpu_streams.py's law and recorder, which go by
a trailing stream parameter, do not see them; this file keeps a recorder, a table and a law of its own: every name of
include/soundml_amd.h matching smx_iir_\\w+_card_f32 has a row here."""
import contextlib
import ctypes as C
import os
import re

import numpy as np
import pytest

from soundml_amd import Iir
from soundml_amd._lib import lib
from conftest import ROOT
from test_gpu_streams import FAST_OFF, H_MS, Case, Placed, hold, ordinary, other, same_bits, sig, streamed      # noqa: F401  (hold is the fixture)

import iir_restatement as R

pytestmark = pytest.mark.gpu

B, W = Iir.BLOCK, Iir.SPAN_BLOCKS
TABLE = {}
ROWS = []


def row(*entries, params=(None,)):
    def mark(fn):
        for p in params:
            for e in entries:
                TABLE.setdefault(e, []).append(fn.__name__)
            ROWS.append((fn, p, frozenset(entries), "%s-%s" % (fn.__name__, "-".join(str(q) for q in (p if isinstance(p, tuple) else (p,))))))
        return fn
    return mark


def header_entries():
    with open(os.path.join(ROOT, "include", "soundml_amd.h")) as fh:
        return sorted(set(re.findall(r"\b(smx_iir_\w+_card_f32)\s*\(", fh.read())))


@contextlib.contextmanager
def recording():
    """every (name, stream handle) one of the header's _card_f32 entries receives: the handle is the second argument"""
    log, saved = [], {}

    def wrap(name, fn):
        def wrapper(*args):
            st = args[1]
            log.append((name, int((st.value if isinstance(st, C.c_void_p) else st) or 0)))
            return fn(*args)
        return wrapper
    try:
        for name in header_entries():
            saved[name] = getattr(lib, name)
            setattr(lib, name, wrap(name, saved[name]))
        yield log
    finally:
        for name, fn in saved.items():
            setattr(lib, name, fn)


def fenced(hold, case, cfg, state, arrays, entries):
    import torch
    side = torch.cuda.Stream()
    assert side.cuda_stream != 0
    p = Placed(side, arrays)
    p.hold(hold, H_MS)
    with recording() as log:
        out, pending, dt = p.run(case, cfg, state)
    side.synchronize()
    wrong = sorted({(n, h) for n, h in log if h != side.cuda_stream})
    assert not wrong, "entry points that were not given the caller's stream %#x: %s" % (side.cuda_stream, wrong)
    assert {n for n, _ in log} == set(entries), "the row declares %s and ran %s" % (sorted(entries), sorted({n for n, _ in log}))
    return out, pending, dt


def config(s, cold=False):
    sos = R.cascade(s).copy()
    if cold:
        sos[0, 0] *= 0.5         # another filter: its block matrix is not on the device yet
    return Iir.Config.create(sos)


N = W * B + 3 * B + 17
SHAPES = [(2, "block"), (2, "general"), (8, "block")]


@row("smx_iir_apply_card_f32", params=SHAPES)
def apply(p):
    return Case([sig(1, 3, N)], lambda c, s, x: Iir.apply(c, x), lambda cold: config(p[0], cold), env=FAST_OFF if p[1] == "general" else None)


@row("smx_iir_apply_card_f32", params=SHAPES[:2])
def apply_with_states(p):
    zi = np.ascontiguousarray(R.batch_state(3, 1, p[0])[0])
    return Case([sig(2, 3, N)], lambda c, s, x: Iir.apply(c, x, zi=zi, return_state=True), lambda cold: config(p[0], cold),
                env=FAST_OFF if p[1] == "general" else None)


@row("smx_iir_apply_card_f32", params=[2])
def apply_with_resident_states(s):
    """one state per channel, given as a device tensor: it is an input like the audio"""
    return Case([sig(4, 3, N), np.ascontiguousarray(R.batch_state(5, 3, s))], lambda c, st, x, z: Iir.apply(c, x, zi=z, return_state=True),
                lambda cold: config(s, cold))


@row("smx_iir_filtfilt_card_f32", params=SHAPES)
def filtfilt(p):
    return Case([sig(6, 3, N)], lambda c, s, x: Iir.filtfilt(c, x), lambda cold: config(p[0], cold), env=FAST_OFF if p[1] == "general" else None)


@row("smx_iir_kernel_step_card_f32", params=SHAPES)
def kernel(p):
    return Case([sig(7, 3, N)], lambda c, k, x: streamed(k, x, [0, 41, W * B + 90, N]), lambda cold: config(p[0], cold),
                lambda c: Iir.Kernel.prepare(c, 3), env=FAST_OFF if p[1] == "general" else None)


IDS = [r[3] for r in ROWS]


@pytest.mark.parametrize("r", ROWS, ids=IDS)
def test_fence(hold, r):
    """warm: the bits of the default stream, the caller's handle in every entry, the result still pending on return"""
    fn, param, entries, name = r
    case = fn(param)
    cfg = case.make(False)
    want = ordinary(case, cfg, case.inputs)
    state = case.state(cfg)
    if state is not None:       # a streaming object is warm on its second pass over the same chunk sizes
        out, _, _ = fenced(hold, case, cfg, state, case.inputs, entries)
        same_bits(out, want, name + " (first pass)")
        state.reset()
    out, pending, dt = fenced(hold, case, cfg, state, case.inputs, entries)
    same_bits(out, want, name)
    assert pending, "%s synchronised the caller's stream (it came back after %.1f ms of a %g ms hold)" % (name, 1e3 * dt, H_MS)
    assert 1e3 * dt <= H_MS / 2, "%s took %.1f ms to return, warm: it builds tables per call or waits for the device" % (name, 1e3 * dt)


@pytest.mark.parametrize("r", ROWS, ids=IDS)
def test_cold_first_use(hold, r):
    """the first launch of a fresh configuration, the upload of its block matrix included, with the side stream current: bits only"""
    fn, param, entries, name = r
    case = fn(param)
    cfg = case.make(True)
    out, _, _ = fenced(hold, case, cfg, case.state(cfg), case.inputs, entries)
    same_bits(out, ordinary(case, cfg, case.inputs), name)


@pytest.mark.parametrize("r", ROWS, ids=IDS)
def test_two_streams(hold, r):
    """one configuration, data A on one stream and B on another, both held, both calls queued: each gets its own bits"""
    import torch
    fn, param, entries, name = r
    case = fn(param)
    cfg = case.make(False)
    data = [case.inputs, [other(a) for a in case.inputs]]
    want = [ordinary(case, cfg, d) for d in data]
    sides = [torch.cuda.Stream(), torch.cuda.Stream()]
    placed = [Placed(s, d) for s, d in zip(sides, data)]
    states = [case.state(cfg) for _ in sides]
    for p in placed:
        p.hold(hold, H_MS)
    got = [p.run(case, cfg, st)[0] for p, st in zip(placed, states)]
    for s in sides:
        s.synchronize()
    for k in (0, 1):
        same_bits(got[k], want[k], "%s on stream %d of two" % (name, k))


def test_coverage_law():
    """every _card_f32 entry of the header runs in a row above, and none of them ends its parameters with the stream (no GPU work)"""
    declared = set(header_entries())
    assert len(declared) >= 3
    missing = sorted(declared - set(TABLE))
    assert not missing, "stream-taking entry points without a row: %s" % ", ".join(missing)
    assert not sorted(set(TABLE) - declared)
    assert len(set(IDS)) == len(IDS)
