"""Cqt.transform / Cqt.power_spectrum / chroma_cqt on the device (soundml_amd/csrc/cqt.hip) against the reference's golden
vectors, against the numpy restatement of cqt.ml (tests/cqt_restatement.py, itself pinned to those vectors by
tests/test_cqt_restatement.py), and the projection kernel alone on exact integer data.

Tolerances are the reference's float32 tiers (cqt_goldens.ml:27-47): this path stores float32 and accumulates in double,
like the reference's float32 cases.  Fractions of the case peak max|expected|: 5e-6 (+ rtol 1e-5) where the plan never
decimates, 6e-4 where it does (two conforming 2:1 filters), and 5e-6 with NO relative term in the composition tests, where
the restatement decimates with the device's own Resample.apply and both sides project the same octave signals."""
import ctypes as C
import functools

import numpy as np
import pytest

import soundml_amd as S
from soundml_amd import Chroma, Cqt, Resample
from soundml_amd._lib import check, lib
from conftest import check_close
from oracle import soundml_oracle as O

import cqt_restatement as R

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

FLOAT32_FRACTION = R.TIGHT32_ATOL   # 5e-6 of peak


def dev(a):
    return torch.from_numpy(np.array(a, copy=True, order="C")).to("cuda:0")


def host(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)


@functools.lru_cache(maxsize=None)
def halver():
    return Resample.Config.create(2, 1, "high")


def device_decimate(y):
    """The library's own public 2:1 conversion on the float32 rounding of ``y`` (host arrays in, host arrays out)."""
    return Resample.apply(halver(), np.ascontiguousarray(y, dtype=np.float32))


def cases(suite, name):
    return [pytest.param(c, id=c["name"]) for c in R.golden_cases(suite, name)]


def float32_signal(params):
    return R.golden_signal(params).astype(np.float32)   # float64 cases are fed the float32 cast


# ---- (a) the golden vectors -----------------------------------------------------------------------------------------------

def replay(case, fraction, rtol):
    p = case["params"]
    c = Cqt.Config.create(**R.golden_kwargs(p))
    got = host(Cqt.power_spectrum(c, dev(float32_signal(p)), power=1.0))
    assert got.dtype == np.float32
    peak = float(np.max(np.abs(case["values"])))
    err = float(np.max(np.abs(got.astype(np.float64).reshape(-1) - np.asarray(case["values"])))) if got.size else 0.0
    print("%s: worst deviation %.3g of peak" % (case["name"], err / peak))
    check_close(got, case["values"], shape=case["shape"], rtol=rtol, atol=fraction * peak, msg=case["name"])


@pytest.mark.parametrize("case", cases("cqt", "cqt_tight"))
def test_tight_goldens(case):
    replay(case, R.TIGHT32_ATOL, R.RTOL)


@pytest.mark.parametrize("case", cases("cqt", "cqt_wide"))
def test_wide_goldens(case):
    replay(case, R.WIDE_ATOL, R.RTOL)


@pytest.mark.parametrize("case", cases("chroma", "chroma_cqt"))
def test_chroma_cqt_goldens(case):
    """chroma_goldens.ml:190-215: 1e-4 of the case peak where the plan decimates, 1e-6 at the odd hop, rtol 1e-5."""
    p = case["params"]
    c = Cqt.Config.create(n_bins=p["n_bins"], sample_rate=p["sample_rate"], fmin=p["fmin"], bins_per_octave=p["bins_per_octave"],
                          tuning=p["tuning"], hop=p["hop"])
    norm = {"inf": "inf", "l2": 2.0, "l1": 1.0, "none": None}[p["norm"]]
    x = dev(float32_signal(p))
    got = host(S.chroma_cqt(c, x, n_chroma=p["n_chroma"], norm=norm))
    fraction = R.CHROMA_CQT_ODD_HOP_ATOL if p["hop"] % 2 == 1 else R.CHROMA_CQT_ATOL
    peak = float(np.max(np.abs(case["values"])))
    print("%s: worst deviation %.3g of peak" % (case["name"], float(np.max(np.abs(got.reshape(-1) - np.asarray(case["values"])))) / peak))
    check_close(got, case["values"], shape=case["shape"], rtol=R.CHROMA_CQT_RTOL, atol=fraction * peak, msg=case["name"])
    # chroma_cqt is of_cqt after the magnitude transform (chroma_props.ml:289-295), bit for bit, host arrays included
    two_steps = Chroma.of_cqt(c, Cqt.power_spectrum(c, x, power=1.0), n_chroma=p["n_chroma"], norm=norm)
    assert np.array_equal(host(two_steps), got)
    assert np.array_equal(S.chroma_cqt(c, host(x), n_chroma=p["n_chroma"], norm=norm), got)


# ---- (b) composition: the restatement on the device's own octave signals ---------------------------------------------------

@functools.lru_cache(maxsize=None)
def clips(n, count=3):
    """``count`` distinct clips of LCG noise with a slow envelope each, float32 [count; n]."""
    base = O.lcg_signal(count * n, R.SEED).reshape(count, n)
    t = np.arange(n, dtype=np.float64) / float(max(n, 1))
    env = np.stack([0.25 + 0.75 * np.cos(2.0 * np.pi * (k + 1) * t) ** 2 for k in range(count)])
    return (base * env * (2.0 ** -np.arange(count))[:, None]).astype(np.float32)


def against_the_restatement(kw, x, fraction=FLOAT32_FRACTION):
    c, r = Cqt.Config.create(**kw), R.Config(**kw)
    want = R.transform(r, x.astype(np.float64), device_decimate)
    got = host(Cqt.transform(c, dev(x)))
    assert got.dtype == np.complex64 and got.shape == want.shape
    if want.size:
        peak = float(np.max(np.abs(want)))
        worst = float(np.max(np.abs(got.astype(np.complex128) - want)))
        print("%r: worst deviation %.3g of peak" % (kw, worst / peak))
        assert worst <= fraction * peak, "worst deviation %.3g of peak" % (worst / peak)
    return c, got


COMPOSITION = {
    "c1_84_hop512": (dict(n_bins=84, sample_rate=22050), 8192),
    "partial_90_hop256": (dict(n_bins=90, sample_rate=22050, hop=256), 4096),
    "bpo36_252": (dict(n_bins=252, sample_rate=22050, bins_per_octave=36), 4096),
    "early_48_scale": (dict(n_bins=48, sample_rate=22050), 8192),
    "early_48_noscale": (dict(n_bins=48, sample_rate=22050, scale=False), 8192),
}


@pytest.mark.parametrize("name", sorted(COMPOSITION))
def test_composition(name):
    kw, n = COMPOSITION[name]
    c, _ = against_the_restatement(kw, clips(n))
    assert c.early > 0 or any(hop % 2 == 0 for _, _, _, hop, _ in c.octaves[:-1])   # these plans decimate
    if name.startswith("early"):
        assert c.early == 3
    if name.startswith("partial"):
        assert c.octaves[-1][1] == 6   # a partial bottom octave


# ---- (c) edges -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [0, 100])
def test_short_signals(n):
    """n = 100 is shorter than every n_fft / 2 of the plan; n = 0 has no frames."""
    kw = dict(n_bins=84, sample_rate=22050)
    c, got = against_the_restatement(kw, clips(n, 2))
    assert got.shape == (2, 84, Cqt.frames(c, n)) == (2, 84, 1 if n else 0)
    assert all(n < n_fft // 2 for _, _, n_fft, _, _ in c.octaves)


@pytest.mark.parametrize("n_bins", [1, 7])
def test_few_bins(n_bins):
    c, got = against_the_restatement(dict(n_bins=n_bins, sample_rate=22050), clips(8192))
    assert c.n_octaves == 1 and got.shape == (3, n_bins, 17)


@pytest.mark.parametrize("pad", ["reflect", "edge"])
@pytest.mark.parametrize("n", [100, 3000])
def test_boundary_rules_at_the_odd_hop(pad, n):
    """hop 511: every octave at the input rate, n_fft up to 16384, so the boundary rule serves most of every frame (n = 100:
    the reflection wraps many times)."""
    against_the_restatement(dict(n_bins=84, sample_rate=22050, hop=511, pad=pad), clips(n, 2) + np.float32(0.5))


def test_constant_padding_with_a_value():
    against_the_restatement(dict(n_bins=48, sample_rate=22050, pad="constant", pad_value=0.25), clips(4096, 2))


def test_empty_leading_axis():
    c = Cqt.Config.create(84, 22050)
    for x in (torch.zeros((2, 0, 4096), device="cuda:0"), np.zeros((2, 0, 4096), dtype=np.float32)):
        assert tuple(Cqt.transform(c, x).shape) == (2, 0, 84, 9)
        assert tuple(Cqt.power_spectrum(c, x).shape) == (2, 0, 84, 9)
        assert tuple(S.chroma_cqt(c, x).shape) == (2, 0, 12, 9)


def test_powers_and_resident_results():
    """|transform|^power in the reference's rounding order (cqt.ml:671-675: the magnitude of the rounded complex64 value in
    float32, then squared / kept / raised): powers 1 and 2 are exact operations, so equal bit for bit; the general power goes
    through pow, allowed four float32 rounding steps.  Host arrays and device tensors give the same bits."""
    c = Cqt.Config.create(90, 22050, hop=256)
    x = clips(4096).reshape(3, 1, 4096)
    z = Cqt.transform(c, dev(x))
    assert z.is_cuda and tuple(z.shape) == (3, 1, 90, 17)
    zh = Cqt.transform(c, x)
    assert isinstance(zh, np.ndarray) and np.array_equal(zh, host(z))
    m = np.sqrt(zh.real.astype(np.float64) ** 2 + zh.imag.astype(np.float64) ** 2).astype(np.float32)
    for power in (1.0, 2.0, 0.5):
        s = Cqt.power_spectrum(c, dev(x), power=power)
        assert s.is_cuda and s.dtype == torch.float32
        assert np.array_equal(Cqt.power_spectrum(c, x, power=power), host(s))
        if power == 1.0:
            assert np.array_equal(host(s), m)
        elif power == 2.0:
            assert np.array_equal(host(s), m * m)
        else:
            want = m.astype(np.float64) ** power
            assert np.all(np.abs(host(s) - want) <= 4.0 * 2.0 ** -24 * want)
    # a batch slice is the batched call's slice
    assert np.array_equal(host(Cqt.transform(c, dev(x[1]))), zh[1])


# ---- (d) the kernel alone, on exact data -------------------------------------------------------------------------------------

def project(x, taps, n_fft, hop, frames, first, n_bins, divisors=None, pad="constant", pad_value=0.0, power=None):
    lead, n = x.shape
    count = taps.shape[0]
    d_x, d_taps = dev(x), dev(np.ascontiguousarray(taps, dtype=np.complex128))
    d_div = dev(divisors) if divisors is not None else None
    out = torch.full((lead, n_bins, frames), -7.0, dtype=torch.complex64 if power is None else torch.float32, device="cuda:0")
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    check(lib.smx_debug_cqt_project_f32_dev(ptr(d_x), lead, n, n, ptr(d_taps), ptr(d_div), count, n_fft, hop, S._lib.PAD[pad], pad_value,
                                            first, n_bins, frames, 0 if power is None else 1, 0.0 if power is None else power, ptr(out),
                                            C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    return host(out)


def lcg_integers(count, lo, hi, seed):
    state, out = seed, np.empty(count, dtype=np.int64)
    for i in range(count):
        state = (1103515245 * state + 12345) % (1 << 31)
        out[i] = lo + (state >> 12) % (hi - lo + 1)
    return out


@pytest.mark.parametrize("count,n_fft,hop,frames", [(1, 1, 1, 5), (12, 256, 512, 17), (12, 256, 8, 33), (37, 512, 3, 19), (5, 32768, 511, 2)])
def test_projection_kernel_is_exact(count, n_fft, hop, frames):
    """Taps in [-3, 3] + i [-3, 3] and samples in [-4, 4]: every partial sum is an integer below 2^24, exact in float64 in any
    order and exact again as complex64.  A wrong lane map, tile edge or frame offset cannot hide behind a tolerance."""
    n = (frames - 1) * hop + max(1, n_fft // 2)
    x = lcg_integers(2 * n, -4, 4, 20260803).reshape(2, n).astype(np.float32)
    g = lcg_integers(2 * count * n_fft, -3, 3, 20260804).reshape(2, count, n_fft)
    taps = g[0] + 1j * g[1]
    first, n_bins = 3, count + 5
    got = project(x, taps, n_fft, hop, frames, first, n_bins)
    xp = R.padded(x.astype(np.float64), n_fft // 2, (frames - 1) * hop + n_fft, "constant", 0.0)
    idx = (np.arange(frames) * hop)[:, None] + np.arange(n_fft)[None, :]
    want = np.einsum("cpn,bn->cbp", xp[:, idx], taps)
    assert np.max(np.abs(want.real)) < 2 ** 24 and np.max(np.abs(want.imag)) < 2 ** 24
    assert np.array_equal(got[:, first:first + count], want.astype(np.complex64))
    untouched = np.delete(got, np.s_[first:first + count], axis=1)
    assert np.array_equal(untouched, np.full_like(untouched, -7.0))   # only the octave's rows are written


def test_projection_kernel_divisors_and_power():
    """Power-of-two divisors keep the data exact: z / d and |z|^2 of integers."""
    count, n_fft, hop, frames = 20, 64, 5, 131    # two bin tiles, two frame tiles, frames sharing samples
    n = (frames - 1) * hop + 7
    x = lcg_integers(2 * n, -4, 4, 7).reshape(2, n).astype(np.float32)
    g = lcg_integers(2 * count * n_fft, -3, 3, 8).reshape(2, count, n_fft)
    taps = g[0] + 1j * g[1]
    divisors = 2.0 ** (np.arange(count) % 4)
    xp = R.padded(x.astype(np.float64), n_fft // 2, (frames - 1) * hop + n_fft, "edge", 0.0)
    idx = (np.arange(frames) * hop)[:, None] + np.arange(n_fft)[None, :]
    want = np.einsum("cpn,bn->cbp", xp[:, idx], taps) / divisors[None, :, None]
    got = project(x, taps, n_fft, hop, frames, 0, count, divisors=divisors, pad="edge")
    assert np.array_equal(got, want.astype(np.complex64))
    got2 = project(x, taps, n_fft, hop, frames, 0, count, divisors=divisors, pad="edge", power=2.0)
    m = np.sqrt(want.real ** 2 + want.imag ** 2).astype(np.float32)
    assert np.array_equal(got2, m * m)
