"""Streams: the Pcen device entry points on a held side stream, by the method of test_gpu_streams.py (the decoy inputs, the hold,
the true inputs copied in behind it, `pending` read at once, the bits after the wait, a warm call back within H / 2).  Those entries
end in `_card_f32` and take the stream directly behind the first argument, so test_gpu_streams.py's law and recorder, which go by a
trailing stream parameter, do not see them; this file keeps a recorder, a table and a law of its own: every name of
include/soundml_amd.h matching smx_pcen_\\w+_card_f32 has a row here.  A row's configuration is its Pcen.Config (and, from audio,
the STFT and mel configurations): the cold one is a configuration nothing else in the process has built or used."""
import contextlib
import ctypes as C
import os
import re

import numpy as np
import pytest

import soundml_amd as S
from soundml_amd import Pcen
from soundml_amd._lib import lib
from conftest import ROOT
from test_gpu_streams import (FAST_OFF, H_MS, SR, Case, Placed, hold, mags, mel_config, ordinary, other, same_bits, sig, stft_config,      # noqa: F401  (hold is the fixture)
                              streamed)

pytestmark = pytest.mark.gpu

TABLE = {}
ROWS = []
LEAD, BANDS, FRAMES = 2, 70, 2 * 64 + 37


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
        return sorted(set(re.findall(r"\b(smx_pcen_\w+_card_f32)\s*\(", fh.read())))


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


def config(cold):
    return Pcen.Config.create(gain=0.8, bias=10.0, power=0.25, scale=2.0 ** 31) if cold else Pcen.Config.create(scale=2.0 ** 31)


ROUTES = ["tile", "general"]


def env_of(route):
    return FAST_OFF if route == "general" else None


@row("smx_pcen_apply_card_f32", params=ROUTES)
def apply(route):
    return Case([mags(1, LEAD, BANDS, FRAMES)], lambda c, s, x: Pcen.apply(c, x), config, env=env_of(route))


@row("smx_pcen_apply_card_f32", params=ROUTES)
def apply_from_a_state(route):
    """the spectrogram and the device-resident state both arrive behind the hold; the final state comes back with the result"""
    return Case([mags(2, LEAD, BANDS, FRAMES), mags(3, LEAD, BANDS, dtype=np.float64)],
                lambda c, s, x, zi: list(Pcen.apply(c, x, zi=zi, return_state=True)), config, env=env_of(route))


@row("smx_pcen_smooth_card_f32", params=ROUTES)
def smooth(route):
    return Case([mags(4, LEAD, BANDS, FRAMES)], lambda c, s, x: Pcen.smooth(c, x), config, env=env_of(route))


@row("smx_pcen_of_audio_card_f32", params=[(2048, 512), (1024, 256)])
def of_audio(p):
    fft, hop = p
    return Case([sig(5, 2, hop * 39 + 17)], lambda c, s, x: S.pcen(c[0], c[1], x, c[2]),
                lambda cold: (stft_config(fft, hop, cold), mel_config(40, SR, fft, cold), config(cold)))


@row("smx_pcen_kernel_step_card_f32", params=ROUTES)
def kernel(route):
    return Case([mags(6, LEAD, BANDS, FRAMES)], lambda c, k, x: streamed(k, x, [0, 5, 64 + 41, FRAMES]), config,
                lambda c: Pcen.Kernel.prepare(c, LEAD, BANDS), env=env_of(route))


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
    """the first launch of a configuration of its own, with the side stream current: bits only"""
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
    assert len(declared) >= 4
    missing = sorted(declared - set(TABLE))
    assert not missing, "stream-taking entry points without a row: %s" % ", ".join(missing)
    assert not sorted(set(TABLE) - declared)
    assert len(set(IDS)) == len(IDS)
    with open(os.path.join(ROOT, "include", "soundml_amd.h")) as fh:
        assert not re.findall(r"\b(smx_pcen\w+)\s*\([^;{}]*?void\s*\*\s*stream\s*\)\s*;", fh.read())
