"""The schedule of the streaming Cqt.Kernel in host integers (cqt_plan.cpp: smx_cqt_config_columns_ready / column_bound /
run_ahead) against a pure-Python simulation of the state machine's counters, and the checks of `prepare` that come before any
device is touched.  Needs the built library, no device.

The simulation is the state machine without the signal: a chain of 2:1 stages that have emitted ``max(0, ceil((fed - K) / 2))``
outputs after ``fed`` inputs (K = 190, the latency of Resample.Config.create(2, 1, "high")), per octave the frames whose last
sample is in (frame p of octave i needs ``p hop_i + n_fft_i / 2`` samples of its stream; under reflect frame 0 also reads sample
``n_fft_i / 2``, so it waits for one more), and the gate: the columns every octave has produced."""
import functools

import numpy as np
import pytest

from soundml_amd import Cqt, Resample
from soundml_amd import _lib

C1 = Cqt.C1

PLANS = {
    "c1_84_hop512": dict(n_bins=84, sample_rate=22050),
    "early_48": dict(n_bins=48, sample_rate=22050),
    "partial_90_hop256": dict(n_bins=90, sample_rate=22050, hop=256),
    "odd_hop63": dict(n_bins=36, sample_rate=22050, fmin=16 * C1, hop=63),
    "hop64": dict(n_bins=36, sample_rate=22050, fmin=16 * C1, hop=64),
    "hop96": dict(n_bins=36, sample_rate=22050, fmin=16 * C1, hop=96),
    "hop24_stops_halving": dict(n_bins=60, sample_rate=22050, fmin=4 * C1, hop=24),
}
PADS = ["constant", "edge", "reflect"]
FEDS = list(range(0, 3001)) + list(range(3037, 60001, 37))


@functools.lru_cache(maxsize=None)
def config(name, pad):
    return Cqt.Config.create(pad=pad, **PLANS[name])


@functools.lru_cache(maxsize=None)
def lag():
    k = Resample.Config.create(2, 1, "high").latency
    assert k == 190
    return k


class Simulation:
    """The counters of the state machine: ``feed(m)`` is a step of m samples; ``produced`` per octave, ``emitted`` the gate."""

    def __init__(self, c):
        self.octaves = c.octaves                      # (first, count, n_fft, hop, halvings), highest octave first
        self.early, self.reflect, self.k = c.early, c.pad == "reflect", lag()
        stages = self.early + self.octaves[-1][4]
        self.fed = [0] * (stages + 1)                 # samples each level of the chain has seen
        self.out = [0] * stages                       # outputs each stage has emitted
        self.produced = [0] * len(self.octaves)
        self.emitted = 0

    def feed(self, m):
        self.fed[0] += m
        for j in range(len(self.out)):
            ready = max(0, -(-(self.fed[j] - self.k) // 2))
            self.fed[j + 1] += ready - self.out[j]
            self.out[j] = ready
        for i, (_, _, n_fft, hop, halvings) in enumerate(self.octaves):
            seen = self.fed[self.early + halvings]
            half = n_fft // 2
            if seen < n_fft - half or (self.reflect and seen < half + 1):
                continue
            self.produced[i] = (seen - (n_fft - half)) // hop + 1
        before, self.emitted = self.emitted, min(self.produced)
        return self.emitted - before


@functools.lru_cache(maxsize=None)
def walk(name, pad):
    """(columns emitted after each of FEDS, the widest spread between two octaves' frame counts on the way)"""
    sim, at, emitted, spread = Simulation(config(name, pad)), 0, [], 0
    for fed in FEDS:
        sim.feed(fed - at)
        at = fed
        emitted.append(sim.emitted)
        spread = max(spread, max(sim.produced) - min(sim.produced))
    return emitted, spread


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("name", sorted(PLANS))
def test_columns_ready_is_the_simulated_gate(name, pad):
    c = config(name, pad)
    want, _ = walk(name, pad)
    got = [Cqt.columns_ready(c, fed) for fed in FEDS]
    assert got == want
    if pad != "reflect":   # the reference's declaration (cqt.mli:199): column p leaves once p hop + latency samples are in
        assert got == [max(0, (fed - c.latency) // c.hop + 1) for fed in FEDS]
    else:                  # frame 0 of an octave waits for one sample more; never earlier than the declaration, one column at most behind it
        declared = [max(0, (fed - c.latency) // c.hop + 1) for fed in FEDS]
        assert all(d - 1 <= g <= d for g, d in zip(got, declared))


def test_the_plans_are_the_ones_meant():
    for name in PLANS:   # the gate opens with the sample that completes `latency`
        c = config(name, "constant")
        assert (Cqt.columns_ready(c, c.latency - 1), Cqt.columns_ready(c, c.latency)) == (0, 1)
    assert config("c1_84_hop512", "constant").latency == 20099
    assert config("partial_90_hop256", "constant").latency == 32195
    assert config("hop64", "constant").latency == 1079
    assert config("early_48", "constant").early == 3
    assert all(o[4] == 0 for o in config("odd_hop63", "constant").octaves)                 # never decimates
    hops = [o[3] for o in config("hop24_stops_halving", "constant").octaves]
    assert hops[-1] % 2 == 1 and hops.count(hops[-1]) >= 2                                   # two octaves share a rate


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("name", sorted(PLANS))
def test_column_bound_covers_every_step_and_the_flush(name, pad):
    c = config(name, pad)
    for max_block in (1, 100, 512, 4096, 22050):
        bound = Cqt.column_bound(c, max_block)
        sim, fed, worst = Simulation(c), 0, 0
        blocks = [max_block] * min(60000 // max_block + 2, 700)
        if max_block == 1:   # single samples around where the gate opens
            sim.feed(c.latency - 300)
            fed = c.latency - 300
        for m in blocks:
            worst = max(worst, sim.feed(m))
            fed += m
            if fed % 7 == 0 or m > 1:   # a flush here returns what is left of Cqt.frames
                worst = max(worst, Cqt.frames(c, fed) - sim.emitted)
        assert worst <= bound, (max_block, worst, bound)
    for n in (0, 1, 100, c.latency - 1, c.latency, c.latency + c.hop):   # a short stream leaves whole at the flush
        assert Cqt.frames(c, n) - Cqt.columns_ready(c, n) <= Cqt.column_bound(c, 1)


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("name", sorted(PLANS))
def test_ring_bound(name, pad):
    """No octave runs further ahead of the slowest than ceil((latency - D_i n_fft_i / 2) / hop) + 1 columns, the worst octave's;
    the column ring holds that plus one step's columns."""
    c = config(name, pad)
    formula = max(-(-(c.latency - (1 << (c.early + halvings)) * (n_fft // 2)) // c.hop) + 1 for _, _, n_fft, _, halvings in c.octaves)
    assert Cqt.run_ahead(c) == formula
    _, spread = walk(name, pad)
    assert spread <= formula
    # within a step: the fastest octave's new frames against the gate before the step
    for max_block in (1, 4096):
        sim, ring = Simulation(c), Cqt.run_ahead(c) + Cqt.column_bound(c, max_block)
        for _ in range(20 if max_block > 1 else 3000):
            before = sim.emitted
            sim.feed(max_block)
            assert max(sim.produced) - before <= ring


def test_prepare_errors_come_before_the_device():
    c = config("c1_84_hop512", "constant")
    with pytest.raises(_lib.InvalidArgument) as e:
        Cqt.Kernel.prepare(c, channels=0, max_block=512)
    assert str(e.value) == "prepare: cannot analyse 0 channels (channels must be at least 1)"
    with pytest.raises(_lib.InvalidArgument) as e:
        Cqt.Kernel.prepare(c, channels=2, max_block=0)
    assert str(e.value) == "prepare: cannot accept blocks of 0 samples (max_block must be at least 1)"
    with pytest.raises(_lib.InvalidArgument) as e:
        Cqt.Kernel.prepare(c, channels=-3, max_block=-1)
    assert str(e.value) == "prepare: cannot analyse -3 channels (channels must be at least 1)"
