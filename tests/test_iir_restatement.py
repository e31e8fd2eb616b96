"""The numpy restatement of Iir (iir_restatement.py) against scipy's pins, no GPU: tests/golden/iir/ holds, for four designed
filters and the K-weighting pair, the sections, one float32 signal of 6000 samples and scipy.signal's float64 sosfilt, sosfilt_zi
and sosfiltfilt (tools/gen_iir_pins.py).  The GPU tests compare the library bit for bit against this restatement; this file
is what ties the restatement to scipy.  Measured figures stand beside each bound (the largest over the pinned filters)."""
import json
import os

import numpy as np
import pytest

import iir_restatement as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "iir")
with open(os.path.join(GOLDEN, "cases.json")) as fh:
    META = json.load(fh)
NAMES = [c["name"] for c in META["cases"]]
HARD = "butter8_lowpass_100hz_48k"          # entries of M reach 8e13 at B = 256

_cache = {}


def pins():
    if "pins" not in _cache:
        with np.load(os.path.join(GOLDEN, "pins.npz")) as z:
            _cache["pins"] = {k: z[k] for k in z.files}
    return _cache["pins"]


def stated(name, block=R.BLOCK):
    key = (name, block)
    if key not in _cache:
        _cache[key] = R.stated(pins()[name + ".sos"], pins()["x"], block=block)[0]
    return _cache[key]


def of_peak(got, want):
    return float(np.max(np.abs(got - want)) / np.max(np.abs(want)))


def test_the_pins_hold_the_cases():
    assert HARD in NAMES and "k_weighting_48k" in NAMES and len(NAMES) == 5
    p = pins()
    assert p["x"].dtype == np.float32 and p["x"].shape == (META["n"],) == (6000,)
    for c in META["cases"]:
        sos = p[c["name"] + ".sos"]
        assert sos.dtype == np.float64 and sos.shape == (c["sections"], 6) and 1 <= c["sections"] <= R.MAX_SECTIONS
        assert p[c["name"] + ".sosfilt"].shape == (6000,) and p[c["name"] + ".sosfiltfilt"].shape == (META["n_filtfilt"],)


@pytest.mark.parametrize("name", NAMES)
def test_serial_order_is_sosfilt(name):
    """bound 1e-13 of peak; measured 0 on every filter"""
    p = pins()
    err = of_peak(R.serial(p[name + ".sos"], p["x"])[0], p[name + ".sosfilt"])
    print("%s: serial vs sosfilt %.3g of peak" % (name, err))
    assert err <= 1e-13


@pytest.mark.parametrize("name", NAMES)
def test_stated_order_at_the_library_block(name):
    """bound 1e-10 of peak; measured at B = 256 at most 1.35e-12 (butter4_highpass_20hz_48k; 1.43e-12 at B = 128, 9.7e-13 at 64)"""
    err = of_peak(stated(name), pins()[name + ".sosfilt"])
    print("%s: stated order vs sosfilt %.3g of peak" % (name, err))
    assert err <= 1e-10


@pytest.mark.parametrize("name", NAMES)
def test_float32_result_is_one_rounding(name):
    """bound 1.2e-7 of peak (2^-23: one rounding of a value at most the peak); measured at most 5.4e-8"""
    err = of_peak(stated(name).astype(np.float32).astype(np.float64), pins()[name + ".sosfilt"])
    print("%s: float32 result vs sosfilt %.3g of peak" % (name, err))
    assert err <= 1.2e-7


@pytest.mark.parametrize("name", NAMES)
def test_zi_closed_form(name):
    """bound 1e-10; measured at most 1.2e-11 (butter4_highpass_20hz_48k)"""
    p = pins()
    err = float(np.max(np.abs(R.zi(p[name + ".sos"]) - p[name + ".sosfilt_zi"])))
    print("%s: zi vs sosfilt_zi %.3g" % (name, err))
    assert err <= 1e-10


@pytest.mark.parametrize("name", NAMES)
def test_filtfilt(name):
    """the stated order against sosfiltfilt: measured at most 7.01e-12 of peak (butter4_highpass_20hz_48k; two serial passes:
    6.85e-12), the bound is ten times that"""
    p = pins()
    x = p["x"][:META["n_filtfilt"]]
    assert R.padlen(p[name + ".sos"]) == {4: 27, 2: 15, 3: 21}[p[name + ".sos"].shape[0]]
    err = of_peak(R.filtfilt(p[name + ".sos"], x)[0], p[name + ".sosfiltfilt"])
    print("%s: filtfilt vs sosfiltfilt %.3g of peak" % (name, err))
    assert err <= 7.01e-11


def partitions(n, B):
    rng = np.random.default_rng(7)
    cuts = sorted(set(rng.integers(0, n + 1, size=12).tolist()) | {0, n})
    yield "seeded", [b - a for a, b in zip(cuts[:-1], cuts[1:])]
    yield "ones across an edge", [B - 3] + [1] * 7 + [0, n - B - 4]
    yield "blocks", [B] * (n // B) + [n % B]
    yield "blocks and one", [B + 1] * (n // (B + 1)) + [n % (B + 1)]
    yield "empties", [0, 5, 0, 0, n - 5, 0]


@pytest.mark.parametrize("name", [HARD, "k_weighting_48k"])
def test_kernel_equals_apply_bit_for_bit(name):
    p = pins()
    B, n = R.BLOCK, 3 * R.BLOCK + 41
    x = np.stack([p["x"][:n], p["x"][n:2 * n] * np.float32(1e-3)])
    want = R.stated(p[name + ".sos"], x)
    for what, sizes in partitions(n, B):
        assert sum(sizes) == n and min(sizes) >= 0
        k = R.Kernel(p[name + ".sos"], 2)
        got, at = [], 0
        for m in sizes:
            out = k.step(x[:, at:at + m])
            assert (out is None) == (m == 0)
            if out is not None:
                got.append(out)
            at += m
        assert k.flush() == []
        assert np.array_equal(np.concatenate(got, axis=1).view(np.int64), want.view(np.int64)), what


def test_another_block_size_gives_other_bits():
    """the bit tests can fail: the grid is part of the result"""
    differ = [name for name in NAMES if not np.array_equal(stated(name, R.BLOCK), stated(name, R.BLOCK // 2))]
    assert differ


def test_state_handed_on():
    """zf of x[:k] as zi of x[k:]: the grid restarts, so to rounding only; on a block edge the bits agree"""
    p = pins()
    sos, x = p[HARD + ".sos"], p["x"][:1000]
    whole = R.stated(sos, x)[0]
    for k in (R.BLOCK * 3, 333):
        head, zf = R.stated(sos, x[:k], return_state=True)
        tail = R.stated(sos, x[k:], zf)[0]
        joined = np.concatenate([head[0], tail])
        if k % R.BLOCK == 0:
            assert np.array_equal(joined, whole)
        assert of_peak(joined, whole) <= 1e-10
