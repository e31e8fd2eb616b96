"""The streaming `Cqt.Kernel` on the device (soundml_amd/csrc/cqt_stream.hip; cqt.mli:317-413): the partition law against the
OFFLINE transform -- the concatenation of every step plus flush equals `Cqt.transform` (with a power: `Cqt.power_spectrum`) of the
concatenated signal BIT FOR BIT under every chunking, which is stronger than the reference's 2e-6 --, the boundary rules, the
emission schedule (`Cqt.columns_ready`), the errors, host and device chunks, reset, independence of two kernels, and two of the
reference's golden cases streamed."""
import functools

import numpy as np
import pytest

from soundml_amd import Cqt
from soundml_amd import _lib
from conftest import check_close
from oracle import soundml_oracle as O

import cqt_restatement as R

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

C1 = Cqt.C1


def dev(a):
    return torch.from_numpy(np.array(a, copy=True, order="C")).to("cuda:0")


def host(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)


@functools.lru_cache(maxsize=None)
def clips(n, count=3):
    """The seeded noise of test_gpu_cqt.py: ``count`` distinct clips of LCG noise with a slow envelope each, float32 [count; n]."""
    base = O.lcg_signal(count * n, R.SEED).reshape(count, n)
    t = np.arange(n, dtype=np.float64) / float(max(n, 1))
    env = np.stack([0.25 + 0.75 * np.cos(2.0 * np.pi * (k + 1) * t) ** 2 for k in range(count)])
    return (base * env * (2.0 ** -np.arange(count))[:, None]).astype(np.float32)


def frozen(**kw):
    return tuple(sorted(kw.items()))


@functools.lru_cache(maxsize=None)
def config(key):
    return Cqt.Config.create(**dict(key))


@functools.lru_cache(maxsize=None)
def offline(key, n, count, offset=0.0, power=None):
    """The offline result the streams are held to, computed once per case and left unchanged."""
    x = clips(n, count) + np.float32(offset)
    c = config(key)
    out = Cqt.transform(c, x) if power is None else Cqt.power_spectrum(c, x, power=power)
    out.setflags(write=False)
    return x, out


def stream(kern, x, cuts, c=None):
    """Every step's result and the flush's; with ``c``, the emission schedule is checked after every step."""
    parts, sizes, total = [], [], 0
    for a, b in zip(cuts[:-1], cuts[1:]):
        y = kern.step(x[..., a:b])
        sizes.append(0 if y is None else int(y.shape[-1]))
        total += sizes[-1]
        if y is not None:
            parts.append(y)
        if c is not None:
            assert total == Cqt.columns_ready(c, b), (b, total)
    y = kern.flush()
    sizes.append(0 if y is None else int(y.shape[-1]))
    if y is not None:
        parts.append(y)
    return parts, sizes


def joined(parts, like):
    if not parts:
        return np.zeros(like.shape[:-1] + (0,), dtype=like.dtype)
    return np.concatenate([host(p) for p in parts], axis=-1)


CHUNKINGS = {
    "one": lambda n, rng: [0, n],
    "halves": lambda n, rng: [0, n // 2, n],
    "small": lambda n, rng: list(range(0, n, 97)) + [n],
    "random": lambda n, rng: [0] + sorted(set(int(v) for v in rng.integers(1, max(2, n), size=12))) + [n],
    "with_empty": lambda n, rng: [0, 0, n // 3, n // 3, n, n],
}

PLANS = {
    "c1_84_hop512": (frozen(n_bins=84, sample_rate=22050), 23017),
    "early_48_scale": (frozen(n_bins=48, sample_rate=22050), 23017),
    "early_48_noscale": (frozen(n_bins=48, sample_rate=22050, scale=False), 23017),
    "partial_90_hop256": (frozen(n_bins=90, sample_rate=22050, hop=256), 40000),
    "odd_hop63": (frozen(n_bins=36, sample_rate=22050, fmin=16 * C1, hop=63), 4096),
    "hop24_stops_halving": (frozen(n_bins=60, sample_rate=22050, fmin=4 * C1, hop=24), 8000),
    "one_octave_early6": (frozen(n_bins=7, sample_rate=22050), 23017),
}


# ---- 5. the partition law against the offline transform -----------------------------------------------------------------------

@pytest.mark.parametrize("chunking", sorted(CHUNKINGS))
@pytest.mark.parametrize("name", sorted(PLANS))
def test_partition_law(name, chunking):
    key, n = PLANS[name]
    c = config(key)
    x, whole = offline(key, n, 3)
    rng = np.random.default_rng(sum(map(ord, name)))
    cuts = CHUNKINGS[chunking](n, rng)
    kern = Cqt.Kernel.prepare(c, channels=3, max_block=n)
    parts, sizes = stream(kern, x, cuts, c)
    got = joined(parts, whole)
    assert got.dtype == np.complex64 and got.shape == whole.shape == (3, c.n_bins, Cqt.frames(c, n))
    assert np.array_equal(got, whole), (chunking, sizes)
    assert kern.flush() is None


def test_the_plans_are_the_ones_meant():
    c = config(PLANS["c1_84_hop512"][0])
    assert c.latency == 20099 and Cqt.columns_ready(c, 23017) == 6 and Cqt.frames(c, 23017) == 45
    assert config(PLANS["early_48_scale"][0]).early == 3 and config(PLANS["early_48_noscale"][0]).early == 3
    c = config(PLANS["partial_90_hop256"][0])
    assert c.latency == 32195 and c.octaves[-1][1] == 6 and c.octaves[-1][2] == 128
    c = config(PLANS["odd_hop63"][0])
    assert [o[2] for o in c.octaves] == [256, 512, 1024] and all(o[4] == 0 for o in c.octaves)
    hops = [o[3] for o in config(PLANS["hop24_stops_halving"][0]).octaves]
    assert hops[-1] % 2 == 1 and hops[-2] == hops[-1]
    c = config(PLANS["one_octave_early6"][0])
    assert c.n_octaves == 1 and c.early == 6


# ---- 6. one-sample chunks --------------------------------------------------------------------------------------------------------

def test_one_sample_chunks():
    key, n = frozen(n_bins=36, sample_rate=22050, fmin=16 * C1, hop=64), 2500
    c = config(key)
    assert c.latency == 1079
    x, whole = offline(key, n, 2)
    kern = Cqt.Kernel.prepare(c, channels=2, max_block=1)
    parts, sizes = stream(kern, dev(x), list(range(n + 1)), c)
    assert max(sizes[:-1]) == 1
    assert np.array_equal(joined(parts, whole), whole)


# ---- 7. boundary rules -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [100, 3000])
@pytest.mark.parametrize("pad", ["reflect", "edge"])
@pytest.mark.parametrize("plan", ["odd_hop63", "c1_84_hop512"])
def test_boundary_rules(plan, pad, n):
    """n = 100 is shorter than every half window: everything leaves at the flush, and the reflection wraps."""
    key = frozen(pad=pad, **dict(PLANS[plan][0]))
    c = config(key)
    x, whole = offline(key, n, 2, 0.5)
    for cuts in ([0, n], list(range(0, n, 37)) + [n]):
        kern = Cqt.Kernel.prepare(c, channels=2, max_block=n)
        parts, sizes = stream(kern, x, cuts, c)
        if n == 100:
            assert all(n < n_fft // 2 for _, _, n_fft, _, _ in c.octaves) and sum(sizes[:-1]) == 0
        assert np.array_equal(joined(parts, whole), whole), (cuts[:4], sizes)


def test_constant_padding_with_a_value():
    key, n = frozen(n_bins=48, sample_rate=22050, pad="constant", pad_value=0.25), 4096
    c = config(key)
    x, whole = offline(key, n, 2)
    kern = Cqt.Kernel.prepare(c, channels=2, max_block=1000)
    parts, _ = stream(kern, x, list(range(0, n, 1000)) + [n], c)
    assert np.array_equal(joined(parts, whole), whole)


@pytest.mark.parametrize("pad", ["constant", "reflect", "edge"])
@pytest.mark.parametrize("n", [0, 1])
def test_empty_and_single_sample(n, pad):
    key = frozen(pad=pad, **dict(PLANS["c1_84_hop512"][0]))
    c = config(key)
    x, whole = offline(key, n, 2, 0.5)
    kern = Cqt.Kernel.prepare(c, channels=2, max_block=16)
    parts, sizes = stream(kern, x, [0, n], c)
    assert sum(sizes) == Cqt.frames(c, n) == n
    assert np.array_equal(joined(parts, whole), whole)


# ---- 8. the emission schedule and the errors -------------------------------------------------------------------------------------

def test_emission_schedule_and_errors():
    key, n = PLANS["c1_84_hop512"]
    c = config(key)
    x, whole = offline(key, n, 3)
    kern = Cqt.Kernel.prepare(c, channels=3, max_block=4096)
    assert kern.latency == c.latency == 20099 and kern.column_bound == Cqt.column_bound(c, 4096)
    with pytest.raises(_lib.InvalidArgument) as e:
        kern.step(x[:, :4097])
    assert str(e.value) == "step: cannot feed a 4097-sample chunk (max_block is 4096)"
    with pytest.raises(_lib.InvalidArgument) as e:
        kern.step(np.float32(1.0))
    assert str(e.value) == "step: cannot analyse a rank-zero tensor (the time axis must exist)"
    with pytest.raises(_lib.InvalidArgument) as e:
        kern.step(x[:, :16].astype(np.float64))
    assert str(e.value) == "step: cannot analyse float64 audio (this path is float32)"
    assert kern.step(x[:, :0]) is None
    parts, sizes = stream(kern, x, list(range(0, n, 4096)) + [n], c)     # the refused chunks left no trace
    assert sum(sizes) == Cqt.frames(c, n) == 45 and sum(sizes[:-1]) == 6 and max(sizes) <= kern.column_bound
    assert np.array_equal(joined(parts, whole), whole)
    assert kern.flush() is None
    for chunk in (x[:, :16], x[:, :0]):
        with pytest.raises(_lib.InvalidArgument) as e:
            kern.step(chunk)
        assert str(e.value) == "step: cannot feed a drained kernel (flush consumed the tail; reset before reusing)"
    with pytest.raises(_lib.InvalidArgument) as e:
        kern.step(x[:2, :16])
    assert "channels" in str(e.value)


# ---- 9. powers -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("power", [1.0, 2.0, 0.5])
def test_powers(power):
    key, n = PLANS["partial_90_hop256"][0], 36000
    c = config(key)
    x, whole = offline(key, n, 3, 0.0, power)
    kern = Cqt.Kernel.prepare(c, channels=3, max_block=5000, power=power)
    parts, _ = stream(kern, x, list(range(0, n, 5000)) + [n], c)
    got = joined(parts, whole)
    assert got.dtype == np.float32 and got.shape == whole.shape
    assert np.array_equal(got, whole)


# ---- 10. host and device chunks, reset, two kernels ------------------------------------------------------------------------------

def test_host_and_device_chunks_reset_and_two_kernels():
    key, n = PLANS["c1_84_hop512"]
    c = config(key)
    x, whole = offline(key, n, 3)
    x = x.reshape(3, 1, n)
    cuts = list(range(0, n, 3000)) + [n]
    on_host = Cqt.Kernel.prepare(c, channels=3, max_block=3000)
    on_device = Cqt.Kernel.prepare(c, channels=3, max_block=3000)
    h_parts, d_parts = [], []
    xd = dev(x)
    for a, b in zip(cuts[:-1], cuts[1:]):   # interleaved: two kernels of one config do not disturb each other
        h, d = on_host.step(x[..., a:b]), on_device.step(xd[..., a:b])
        assert (h is None) == (d is None)
        if h is not None:
            assert isinstance(h, np.ndarray) and d.is_cuda and d.dtype == torch.complex64 and tuple(d.shape) == h.shape
            assert h.shape[:2] == (3, 1)
            h_parts.append(h)
            d_parts.append(d)
    h, d = on_host.flush(), on_device.flush()
    assert isinstance(h, np.ndarray) and d.is_cuda            # the drain stays where the stream was fed
    got_h, got_d = joined(h_parts + [h], h), joined(d_parts + [d], h)
    assert np.array_equal(got_h, whole.reshape(3, 1, 84, -1)) and np.array_equal(got_d, got_h)
    # reset, then a second signal: as a fresh kernel
    y, whole_y = offline(key, 9001, 3)
    on_device.reset()
    parts, _ = stream(on_device, dev(y), [0, 2999, 5000, 8000, 9001], c)
    assert all(p.is_cuda for p in parts)
    assert np.array_equal(joined(parts, whole_y), whole_y)


# ---- 11. the reference's goldens, streamed ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("suite,name,fraction", [("cqt_wide", "w1_cqt84_hop512_float32", R.WIDE_ATOL),
                                                 ("cqt_tight", "t1_cqt84_hop511_float32", R.TIGHT32_ATOL)])
def test_goldens_streamed(suite, name, fraction):
    """One decimating and one tight case of the reference's vectors in chunks of 1000, at the tolerance test_gpu_cqt.py holds
    the offline path to for that suite."""
    case = next(c for c in R.golden_cases("cqt", suite) if c["name"] == name)
    p = case["params"]
    c = Cqt.Config.create(**R.golden_kwargs(p))
    x = R.golden_signal(p).astype(np.float32)
    n = x.shape[-1]
    kern = Cqt.Kernel.prepare(c, channels=1, max_block=1000, power=1.0)
    parts, _ = stream(kern, dev(x.reshape(1, n)), list(range(0, n, 1000)) + [n], c)
    got = joined(parts, np.zeros((1, c.n_bins, 0), np.float32))[0]
    assert got.dtype == np.float32
    peak = float(np.max(np.abs(case["values"])))
    check_close(got, case["values"], shape=case["shape"], rtol=R.RTOL, atol=fraction * peak, msg=case["name"])
