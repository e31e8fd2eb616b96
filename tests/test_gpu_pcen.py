"""Pcen on the GPU against the numpy restatement (pcen_restatement.py, tied to scipy's lfilter and to librosa's expressions by
test_pcen_restatement.py).  The shapes hit the tile kernel's edges: rows that are no multiple of 64, partial last tiles, one row and
one frame (the general kernel: fewer than Pcen.TILE_MIN_FRAMES frames); every parameter set runs at scale 1 and 2**31.

The gates.  The smoother and the state hold only products and sums: bit for bit.  The compression goes through exp, log, log1p and
expm1, which on the device and in the platform's libm each hold a few float64 ulps; the chain amplifies that to below 1e-13
relative, so a float32 result may differ from the float32-rounded restatement by one float32 ulp where a rounding flips, and nowhere
by more.  The share of cells that differ at all is capped at 1e-3 (pooled over the shapes of a parameter set, and in every shape of
at least a thousand cells, where one cell is less than the cap), so the bound cannot hide a wrong expression.  Float64 host arrays:
check_close at 1e-12 / 1e-15.  Measured on an MI355X: profiles/pcen/NOTES.md."""
import contextlib
import ctypes as C
import functools
import os

import numpy as np
import pytest

import soundml_amd as S
from soundml_amd import Mel, Pcen, Stft
from soundml_amd._lib import check, lib
from conftest import F64_STRICT_ATOL, F64_STRICT_RTOL, check_close

import pcen_restatement as R

pytestmark = pytest.mark.gpu

CASES = [(name, scale) for name in R.SETS for scale in R.SCALES]
IDS = ["%s-scale%g" % c for c in CASES]
SEED = 7


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


@functools.lru_cache(maxsize=None)
def expected(name, scale, shape):
    """-> (S float32, P, M, zf float64), computed once and left unchanged"""
    x = R.inputs(SEED, *shape)
    out = (x,) + R.pcen(x, **dict(R.SETS[name], scale=scale))
    for a in out:
        a.setflags(write=False)
    return out


def config(name, scale):
    return Pcen.Config.create(**dict(R.SETS[name], scale=scale))


def device(a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).cuda()       # a copy: the cached cases are read-only


def host(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)


def same(got, want, what):
    got, want = np.ascontiguousarray(host(got)), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, got.dtype, want.shape, want.dtype)
    word = np.int32 if got.dtype.itemsize == 4 else np.int64
    differ = got.view(word) != want.view(word)
    assert not differ.any(), "%s: %d/%d values differ, the first at %s" % (what, int(differ.sum()), differ.size, np.argwhere(differ)[0].tolist())


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_smoother_and_state_bit_for_bit(case):
    c = config(*case)
    for shape in R.SHAPES:
        x, _, M, zf = expected(*case, shape)
        for name in ("tile", "general"):
            with route(name):
                what = "%s %s" % (shape, name)
                same(Pcen.smooth(c, device(x)), M.astype(np.float32), what + " smooth, device")
                same(Pcen.smooth(c, x), M.astype(np.float32), what + " smooth, host float32")
                same(Pcen.smooth(c, x.astype(np.float64)), M, what + " smooth, host float64")
                same(Pcen.apply(c, device(x), return_state=True)[1], zf, what + " zf, device")
                same(Pcen.apply(c, x, return_state=True)[1], zf, what + " zf, host float32")
                same(Pcen.apply(c, x.astype(np.float64), return_state=True)[1], zf, what + " zf, host float64")


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_apply_float32_within_one_ulp(case):
    c = config(*case)
    differing = cells = 0
    for shape in R.SHAPES:
        x, P, _, _ = expected(*case, shape)
        want = P.astype(np.float32)
        got = host(Pcen.apply(c, device(x)))
        assert got.shape == want.shape and got.dtype == np.float32
        off = np.abs(got.astype(np.float64) - want.astype(np.float64))
        ulps = off / np.spacing(np.abs(want)).astype(np.float64)
        differ = int((got != want).sum())
        print("%s %s: %d of %d cells differ, %.3g float32 ulp at most" % (case, shape, differ, want.size, float(ulps.max())))
        assert np.isfinite(got).all() and (ulps <= 1.0).all(), (shape, float(ulps.max()), np.argwhere(ulps > 1.0)[:1].tolist())
        if want.size >= 1000:
            assert differ <= 1e-3 * want.size, (shape, differ, want.size)
        differing, cells = differing + differ, cells + want.size
    assert differing <= 1e-3 * cells, (differing, cells)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_apply_float64_host_arrays(case):
    c = config(*case)
    worst = 0.0
    for shape in R.SHAPES:
        x, P, _, _ = expected(*case, shape)
        got = Pcen.apply(c, x.astype(np.float64))
        assert got.dtype == np.float64
        live = P != 0
        if live.any():
            worst = max(worst, float((np.abs(got[live] - P[live]) / np.abs(P[live])).max()))
        check_close(got, P, shape=shape, rtol=F64_STRICT_RTOL, atol=F64_STRICT_ATOL, msg="%s %s" % (case, shape))
    print("%s: float64 relative %.3g at most" % (case, worst))


def padded_call(c, x, pad):
    """the device entry on rows `frames + pad` elements apart -> (out, zf)"""
    import torch
    rows, frames = int(np.prod(x.shape[:-1])), x.shape[-1]
    wide = torch.full((rows, frames + pad), float("nan"), dtype=torch.float32, device="cuda")
    wide[:, :frames] = device(x).reshape(rows, frames)
    out = torch.empty(x.shape, dtype=torch.float32, device="cuda")
    zf = torch.empty(x.shape[:-1], dtype=torch.float64, device="cuda")
    ptr = lambda t: C.c_void_p(t.data_ptr())
    check(lib.smx_pcen_apply_card_f32(c._h, C.c_void_p(torch.cuda.current_stream().cuda_stream), ptr(wide), rows, frames, frames + pad, None, ptr(out),
                                      ptr(zf)))
    torch.cuda.synchronize()
    return out, zf


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_every_way_to_the_same_bits(case):
    """the tile and the general route, a leading slice of a batch, the host and the device face, a row-padded input, and a call
    continued from a zf"""
    c = config(*case)
    for shape in R.SHAPES:
        x = expected(*case, shape)[0]
        plain, zf = Pcen.apply(c, device(x), return_state=True)
        plain, zf = host(plain), host(zf)
        what = "%s %s: " % (case, shape)
        with route("general"):
            g, gz = Pcen.apply(c, device(x), return_state=True)
            same(g, plain, what + "the general route")
            same(gz, zf, what + "the general route's zf")
            same(Pcen.apply(c, x), plain, what + "the host face on the general route")
        same(Pcen.apply(c, x), plain, what + "the host face")
        same(Pcen.apply(c, device(x[:1])), plain[:1], what + "a leading slice")
        same(Pcen.apply(c, device(x[0, :1])), plain[0, :1], what + "one row")
        for pad in (1, 3):
            out, z = padded_call(c, x, pad)
            same(out, plain, what + "rows %d elements further apart" % pad)
            same(z, zf, what + "their zf")
        frames = shape[-1]
        for cut in sorted({1, frames // 2, frames - 1} - {0, frames}):
            for on in (device, np.array):
                head, z = Pcen.apply(c, on(x[..., :cut]), return_state=True)
                tail, z2 = Pcen.apply(c, on(x[..., cut:]), zi=z, return_state=True)
                same(np.concatenate([host(head), host(tail)], axis=-1), plain, what + "continued at %d" % cut)
                same(z2, zf, what + "continued at %d, zf" % cut)
        # a host state for a device call and a device state for a device call are the same state
        if frames > 1:
            z = host(Pcen.apply(c, device(x[..., :1]), return_state=True)[1])
            same(Pcen.apply(c, device(x[..., 1:]), zi=z), plain[..., 1:], what + "a host zi on the device face")


@pytest.mark.parametrize("fft,hop,n_mels", [(2048, 512, 128), (1024, 256, 40), (400, 160, 23)])
def test_pcen_of_audio_is_its_composition(fft, hop, n_mels):
    sc = Stft.Config.create(fft_size=fft, hop=hop)
    mc = Mel.Config.create(n_mels=n_mels, sample_rate=22050, fft_size=fft)
    c = Pcen.Config.create(hop=hop, scale=2.0 ** 31)
    x = np.random.default_rng(3).uniform(-1, 1, size=(2, 3, hop * 70 + 17)).astype(np.float32)
    for name in ("tile", "general"):
        with route(name):
            for on in (device, np.array, lambda a: np.array(a, dtype=np.float64)):
                xs = on(x)
                got = S.pcen(sc, mc, xs, c)
                want = Pcen.apply(c, S.mel_spectrogram(sc, mc, xs, power=1.0))
                assert tuple(got.shape) == (2, 3, n_mels, Stft.frames(sc, x.shape[-1]))
                same(got, host(want), "pcen(%d, %d) on the %s route" % (fft, hop, name))
    assert S.pcen(sc, mc, device(x[:0]), c).shape == (0, 3, n_mels, Stft.frames(sc, x.shape[-1]))


def test_unspecified_cells_do_not_fault():
    """negative and non-finite cells are outside the definition: the call completes and the rows without them keep their bits"""
    import torch
    c = Pcen.Config.create()
    x = np.array(expected("defaults", 1.0, (3, 43, 321))[0])
    plain = host(Pcen.apply(c, device(x)))
    x[0, 0, 5], x[0, 1, 7], x[0, 2, 9], x[0, 3, 0] = -1.0, np.nan, np.inf, -np.inf
    for name in ("tile", "general"):
        with route(name):
            got = host(Pcen.apply(c, device(x)))
            torch.cuda.synchronize()
            same(got[1:], plain[1:], "the other slices, %s" % name)
            same(got[0, 4:], plain[0, 4:], "the other rows, %s" % name)
