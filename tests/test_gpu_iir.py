"""Iir on the GPU: every face (host float32, host float64, device float32) bit for bit against the numpy restatement
(iir_restatement.py, tied to scipy by test_iir_restatement.py).  The lengths walk every path of the launcher: shorter than a block
(the general kernel alone), whole blocks with and without a tail, one wave's span of SPAN_BLOCKS blocks to the sample, and more than
two spans; the channel counts pass what one workgroup of the general kernel (64) and of the state chain (64 / 2S rounded) holds.
Each batch holds channels as drawn, scaled by 1e-6 and by 1e6.  The restatement runs once per (S, length) on 65 channels and the
leading shapes take slices of it."""
import contextlib
import os

import numpy as np
import pytest

from soundml_amd import Iir

import iir_restatement as R

pytestmark = pytest.mark.gpu

B, W = Iir.BLOCK, Iir.SPAN_BLOCKS
SHORT = [1, 2, B - 1, B, B + 1, W * B - 1, W * B, W * B + 1]
LONG = 2 * W * B + B + 3
CASES = [(s, n) for s in (1, 2, 4, 8) for n in SHORT] + [(s, LONG) for s in (1, 2)]
LEADS = [(), (3,), (2, 5), (65,)]
CHANNELS = 65
SEED = 11


@contextlib.contextmanager
def route(name):
    saved = os.environ.get("SMX_DISABLE_FAST")
    if name == "general":
        os.environ["SMX_DISABLE_FAST"] = "1"
    else:
        os.environ.pop("SMX_DISABLE_FAST", None)
    try:
        yield
    finally:
        if saved is None:
            os.environ.pop("SMX_DISABLE_FAST", None)
        else:
            os.environ["SMX_DISABLE_FAST"] = saved


def same(got, want, what):
    if hasattr(got, "cpu"):
        got = got.cpu().numpy()
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, got.dtype, want.shape, want.dtype)
    word = np.int32 if got.dtype.itemsize == 4 else np.int64
    differ = got.view(word) != want.view(word)
    assert not differ.any(), "%s: %d/%d values differ from the restatement, the first at %s" % (
        what, int(differ.sum()), differ.size, np.argwhere(differ)[0].tolist())


def shaped(a, lead, tail):
    """the first prod(lead) channels of a [65; ...] array under the leading shape"""
    count = int(np.prod(lead, dtype=np.int64))
    return np.ascontiguousarray(a[:count]).reshape(tuple(lead) + tuple(tail))


def device(a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).cuda()       # a copy: the cached cases are read-only


def config(s):
    return Iir.Config.create(R.cascade(s))


@pytest.mark.parametrize("s,n", CASES)
def test_apply_every_face_and_route(s, n):
    c = config(s)
    x = R.batch(SEED, CHANNELS, n)
    want, zf = R.expected(s, SEED, CHANNELS, n)
    for lead in LEADS:
        x32 = shaped(x, lead, (n,))
        w64, w32 = shaped(want, lead, (n,)), shaped(want.astype(np.float32), lead, (n,))
        wz = shaped(zf, lead, (s, 2))
        for name in ("block", "general"):
            with route(name):
                what = (s, n, lead, name)
                same(Iir.apply(c, device(x32)), w32, what + ("device float32",))
                if lead in ((), (65,)) and name == "general":
                    continue
                same(Iir.apply(c, x32), w32, what + ("host float32",))
                y, z = Iir.apply(c, x32.astype(np.float64), return_state=True)
                same(y, w64, what + ("host float64",))
                same(z, wz, what + ("host float64 state",))


def test_the_routes_agree_and_a_slice_equals_the_batch():
    import torch
    n = 3 * B + 17
    for s in (1, 3, 5, 8):
        c = config(s)
        x = device(R.batch(SEED + 2, CHANNELS, n))
        with route("block"):
            block, zb = Iir.apply(c, x, return_state=True)
            head = Iir.apply(c, x[:7])
        with route("general"):
            general, zg = Iir.apply(c, x, return_state=True)
        assert torch.equal(block.view(torch.int32), general.view(torch.int32)) and torch.equal(zb.view(torch.int64), zg.view(torch.int64)), s
        assert torch.equal(head.view(torch.int32), block[:7].view(torch.int32)), s
        same(block, R.expected(s, SEED + 2, CHANNELS, n)[0].astype(np.float32), (s, "odd section counts"))


@pytest.mark.parametrize("s,n", [(2, B + 1), (4, W * B + 1), (1, 5)])
def test_initial_state_per_call_and_per_channel(s, n):
    c = config(s)
    x = R.batch(SEED, CHANNELS, n)
    for kind in ("call", "rows"):
        want, zf = R.expected(s, SEED, CHANNELS, n, kind)
        zi = R.batch_state(SEED + 1, 1, s)[0] if kind == "call" else R.batch_state(SEED + 1, CHANNELS, s)
        for lead in ((3,), (2, 5), (65,)):
            z = zi if kind == "call" else shaped(zi, lead, (s, 2))
            x32 = shaped(x, lead, (n,))
            for name in ("block", "general"):
                with route(name):
                    what = (s, n, kind, lead, name)
                    y, state = Iir.apply(c, device(x32), zi=z, return_state=True)
                    same(y, shaped(want.astype(np.float32), lead, (n,)), what + ("device",))
                    same(state, shaped(zf, lead, (s, 2)), what + ("device state",))
                    if kind == "rows":
                        y = Iir.apply(c, device(x32), zi=device(z))
                        same(y, shaped(want.astype(np.float32), lead, (n,)), what + ("device, resident zi",))
                    y, state = Iir.apply(c, x32.astype(np.float64), zi=z, return_state=True)
                    same(y, shaped(want, lead, (n,)), what + ("host float64",))
                    same(state, shaped(zf, lead, (s, 2)), what + ("host state",))
                    same(Iir.apply(c, x32, zi=z), shaped(want.astype(np.float32), lead, (n,)), what + ("host float32",))


def test_a_state_handed_on_continues_the_signal():
    """zf of x[:k] as zi of x[k:]: the block grid restarts at k, so to 1e-10 of the peak, not bitwise"""
    n = 5 * B + 9
    for s in (2, 8):
        c = config(s)
        x = shaped(R.batch(SEED + 3, CHANNELS, n), (3,), (n,)).astype(np.float64)
        whole = Iir.apply(c, x)
        for k in (2 * B, B + 37, 3):
            head, zf = Iir.apply(c, x[:, :k], return_state=True)
            tail = Iir.apply(c, x[:, k:], zi=zf)
            joined = np.concatenate([head, tail], axis=1)
            peak = np.max(np.abs(whole), axis=1, keepdims=True)
            err = float(np.max(np.abs(joined - whole) / peak))
            print("S %d, cut at %d: %.3g of peak" % (s, k, err))
            assert err <= 1e-10, (s, k, err)


FILTFILT = [(s, n) for s in (1, 2, 4, 8) for n in ("padlen+1", B + 1)] + [(s, 2 * W * B + 3) for s in (1, 2)]


@pytest.mark.parametrize("s,n", FILTFILT)
def test_filtfilt(s, n):
    c = config(s)
    n = c.padlen + 1 if n == "padlen+1" else n
    channels = 10
    x = R.batch(SEED + 4, channels, n)
    want = R.expected_filtfilt(s, SEED + 4, channels, n)
    for lead in ((), (3,), (2, 5)):
        x32 = shaped(x, lead, (n,))
        w64, w32 = shaped(want, lead, (n,)), shaped(want.astype(np.float32), lead, (n,))
        for name in ("block", "general"):
            with route(name):
                what = (s, n, lead, name)
                same(Iir.filtfilt(c, device(x32)), w32, what + ("device float32",))
                same(Iir.filtfilt(c, x32), w32, what + ("host float32",))
                same(Iir.filtfilt(c, x32.astype(np.float64)), w64, what + ("host float64",))


def test_device_float64_is_refused():
    import soundml_amd as S
    c = config(2)
    x = device(np.zeros((2, 64), np.float64))
    for fn in (Iir.apply, Iir.filtfilt, lambda c_, t: Iir.Kernel.prepare(c_, 2).step(t)):
        with pytest.raises(S.Failure, match="device-resident float64 audio is not supported; pass a host array"):
            fn(c, x)
