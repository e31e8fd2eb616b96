"""Loudness.Meter: under seeded partitions of one signal the concatenated steps equal `momentary` of the whole signal and the reads
equal `integrated` / `short_term` of it, bit for bit: chunks of one sample, chunks that end inside an Iir block and inside a
gating step, an empty chunk, device chunks and host chunks."""
import numpy as np
import pytest

from soundml_amd import Iir, Loudness

import loudness_restatement as R

pytestmark = pytest.mark.gpu

RATE = 8000                      # 30 steps are 24000 samples: short-term windows exist within a short signal
N = 4 * RATE + 777
B = Iir.BLOCK
STEP = R.step(RATE)


def device(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)


def same(got, want, what):
    got, want = np.ascontiguousarray(host(got)), np.ascontiguousarray(host(want))
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape)
    assert np.array_equal(got.view(np.int32), want.view(np.int32)), "%s: %d values differ" % (what, int((got.view(np.int32) != want.view(np.int32)).sum()))


def signal():
    return R.noise(41, 1, 2, N)[0] * np.float32(0.5)


def partitions():
    rng = np.random.default_rng(3)
    cuts = [
        [0, N],
        [0, 1, 2, 3, B - 1, B, B + 1, STEP - 1, STEP, STEP + 1, 4 * STEP - 1, 4 * STEP, 4 * STEP + 1, 4 * STEP + 1, N - 1, N],      # single samples, an empty chunk
        [0, 41, 41 + 64 * B + 90, 30 * STEP + 5, N],                                                                            # heads inside a block, whole spans
        [0] + sorted(rng.choice(np.arange(1, N), size=23, replace=False).tolist()) + [N],
        [0] + list(range(STEP // 2, N, STEP)) + [N],                                                                            # every chunk ends inside a step
    ]
    return cuts


def run(meter, x, cuts, place):
    parts = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        out = meter.step(place(x[:, a:b]))
        assert (out is None) == (max(0, b // STEP - 3) == max(0, a // STEP - 3)), (a, b)
        if out is not None:
            assert out.shape == (max(0, b // STEP - 3) - max(0, a // STEP - 3),)
            parts.append(host(out))
    return np.concatenate(parts, axis=-1)


@pytest.mark.parametrize("p", range(5))
def test_every_chunking_gives_the_offline_bits(p):
    x = signal()
    want_m, want_i, want_s = Loudness.momentary(device(x), RATE), Loudness.integrated(device(x), RATE), Loudness.short_term(device(x), RATE)
    assert want_s.shape[-1] == R.blocks(RATE, N) - 26 >= 2
    cuts = partitions()[p]
    meter = Loudness.Meter.prepare(RATE, 2)
    same(run(meter, x, cuts, device), want_m, "device chunks, partition %d" % p)
    assert meter.position == N and meter.blocks == R.blocks(RATE, N)
    same(meter.integrated(), want_i, "integrated()")
    same(meter.short_term(), want_s, "short_term()")
    meter.reset()                                           # both grids restart
    assert meter.position == 0
    same(run(meter, x, cuts, lambda c: np.ascontiguousarray(c)), want_m, "host chunks after reset, partition %d" % p)
    same(meter.integrated(), want_i, "integrated() from host chunks")
    same(meter.short_term(), want_s, "short_term() from host chunks")


def test_reads_at_any_time_and_a_batch_of_meters():
    """a lead axis, the weights, and a read in the middle of the stream: what the offline faces give for the samples so far"""
    x = np.array(R.noise(42, 3, 2, N)) * np.array([1.0, 0.1, 1e-4], np.float32)[:, None, None]
    weights = (1.0, 1.41)
    meter = Loudness.Meter.prepare(RATE, 3, 2, weights=weights)
    cut = 33 * STEP + 129
    first = meter.step(device(x[..., :cut]))
    same(first, Loudness.momentary(device(x[..., :cut]), RATE, weights=weights), "the first chunk")
    same(meter.integrated(), Loudness.integrated(device(x[..., :cut]), RATE, weights=weights), "integrated() in the middle")
    same(meter.short_term(), Loudness.short_term(device(x[..., :cut]), RATE, weights=weights), "short_term() in the middle")
    rest = meter.step(device(x[..., cut:]))
    same(np.concatenate([host(first), host(rest)], axis=-1), Loudness.momentary(device(x), RATE, weights=weights), "both chunks")
    same(meter.integrated(), Loudness.integrated(device(x), RATE, weights=weights), "integrated() at the end")
    assert meter.flush() == []


def test_the_step_buffer_grows_by_shape_alone():
    """more steps than the first capacity (64), fed in chunks: the doubling keeps what was there"""
    n = 70 * STEP + 11
    x = R.noise(43, 1, 1, n)[0]
    meter = Loudness.Meter.prepare(RATE, 1)
    parts = [meter.step(device(x[:, a:b])) for a, b in ((0, 10 * STEP), (10 * STEP, 63 * STEP + 5), (63 * STEP + 5, 66 * STEP), (66 * STEP, n))]
    same(np.concatenate([host(p) for p in parts], axis=-1), Loudness.momentary(device(x), RATE), "seventy steps")
    same(meter.integrated(), Loudness.integrated(device(x), RATE), "integrated() behind the growth")
