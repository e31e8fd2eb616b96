"""Streams: the Loudness device entry points on a held side stream, by the method of test_gpu_streams.py (the decoy inputs, the
hold, the true inputs copied in behind it, `pending` read at once, the bits after the wait, a warm call back within H / 2).  Those
entries end in `_card_f32` and take the stream directly behind the first argument, so test_gpu_streams.py's law and recorder, which
go by a trailing stream parameter, do not see them; this file keeps a recorder, a table and a law of its own: every name of
include/soundml_amd.h matching smx_loudness_\\w+_card_f32 has a row here.  A row's configuration is its sample rate: the cold one
is a rate whose cascade and block matrix nothing else in the process has built."""
import contextlib
import ctypes as C
import os
import re

import numpy as np
import pytest

from soundml_amd import Iir, Loudness
from soundml_amd._lib import lib
from conftest import ROOT
from test_gpu_streams import FAST_OFF, H_MS, Case, Placed, hold, ordinary, other, same_bits, sig, streamed      # noqa: F401  (hold is the fixture)

pytestmark = pytest.mark.gpu

B, W = Iir.BLOCK, Iir.SPAN_BLOCKS
TABLE = {}
ROWS = []
RATE, COLD_RATE = 8000, 8100
N = W * B + RATE + 17               # a wave's span and more, a tail, and 30 steps: one short-term window at either rate
WEIGHTS = (1.0, 0.5)


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
        return sorted(set(re.findall(r"\b(smx_loudness_\w+_card_f32)\s*\(", fh.read())))


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


def rate_of(cold):
    return COLD_RATE if cold else RATE


ROUTES = ["block", "general"]


def env_of(route):
    return FAST_OFF if route == "general" else None


@row("smx_loudness_block_energy_card_f32", params=ROUTES)
def block_energy(route):
    return Case([sig(1, 3, 2, N)], lambda rate, s, x: Loudness.block_energy(x, rate), rate_of, env=env_of(route))


@row("smx_loudness_momentary_card_f32", params=ROUTES)
def momentary(route):
    return Case([sig(2, 3, 2, N)], lambda rate, s, x: Loudness.momentary(x, rate, weights=WEIGHTS), rate_of, env=env_of(route))


@row("smx_loudness_momentary_card_f32")
def short_term(_):
    return Case([sig(3, 3, 2, N)], lambda rate, s, x: Loudness.short_term(x, rate), rate_of)


@row("smx_loudness_integrated_card_f32", params=ROUTES)
def integrated(route):
    return Case([sig(4, 3, 2, N)], lambda rate, s, x: Loudness.integrated(x, rate, weights=WEIGHTS), rate_of, env=env_of(route))


@row("smx_loudness_integrated_card_f32")
def gate_mask(_):
    import torch
    return Case([sig(5, 3, 2, N)], lambda rate, s, x: Loudness.gate_mask(x, rate).to(torch.int32), rate_of)


@row("smx_loudness_true_peak_card_f32")
def true_peak(_):
    return Case([sig(6, 3, 2, N)], lambda rate, s, x: Loudness.true_peak(x), rate_of)


@row("smx_loudness_normalize_card_f32", params=[None, 0.1])
def normalize(ceiling):
    return Case([sig(7, 3, 2, N)], lambda rate, s, x: Loudness.normalize(x, rate, peak_ceiling=ceiling, weights=WEIGHTS), rate_of)


@row("smx_loudness_meter_step_card_f32", "smx_loudness_meter_read_card_f32", params=ROUTES)
def meter(route):
    def run(rate, k, x):
        return [streamed(k, x, [0, 41, W * B + 90, N]), k.integrated(), k.short_term()]
    return Case([sig(8, 3, 2, N)], run, rate_of, lambda rate: Loudness.Meter.prepare(rate, 3, 2, weights=WEIGHTS), env=env_of(route))


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
    """the first launch at a rate of its own, the upload of its block matrix included, with the side stream current: bits only"""
    fn, param, entries, name = r
    case = fn(param)
    cfg = case.make(True)
    out, _, _ = fenced(hold, case, cfg, case.state(cfg), case.inputs, entries)
    same_bits(out, ordinary(case, cfg, case.inputs), name)


@pytest.mark.parametrize("r", ROWS, ids=IDS)
def test_two_streams(hold, r):
    """data A on one stream and B on another, both held, both calls queued: each gets its own bits"""
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
    assert len(declared) >= 7
    missing = sorted(declared - set(TABLE))
    assert not missing, "stream-taking entry points without a row: %s" % ", ".join(missing)
    assert not sorted(set(TABLE) - declared)
    assert len(set(IDS)) == len(IDS)
