"""Pcen.Kernel on the GPU: under every chunking the concatenated steps equal Pcen.apply of the whole spectrogram bit for bit and the
kernel's final state equals zf, on host chunks and on device chunks, and again after reset.  The state stays on the device and has
no accessor: it is read through what it does, a further step of a few frames must equal Pcen.apply of those frames from zf.
The chunkings walk single frames, the tile width and its neighbours, chunks on either side of the route threshold (Pcen.TILE_MIN_FRAMES: shorter chunks take the
general kernel) and a zero-length chunk in the middle."""
import numpy as np
import pytest

from soundml_amd import Pcen

import pcen_restatement as R

pytestmark = pytest.mark.gpu

T = Pcen.TILE_MIN_FRAMES
LEAD, BANDS, FRAMES = 2, 43, 321
CHUNKINGS = {
    "ones": [1] * 70,
    "tile-edges": [1, 63, 1, 64, 65, None],
    "whole": [None],
    "threshold": [T - 1, T, T + 1, 1, T - 1, 2 * T, None],
    "empty-in-the-middle": [40, 0, 7, 0, None],
}
SETS = ["defaults", "power0", "bias0"]


def device(a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).cuda()


def host(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)


def same(got, want, what):
    got, want = np.ascontiguousarray(host(got)), np.ascontiguousarray(host(want))
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, got.dtype, want.shape, want.dtype)
    word = np.int32 if got.dtype.itemsize == 4 else np.int64
    differ = got.view(word) != want.view(word)
    assert not differ.any(), "%s: %d/%d values differ, the first at %s" % (what, int(differ.sum()), differ.size, np.argwhere(differ)[0].tolist())


def cuts(sizes, total):
    at, out = 0, []
    for s in sizes:
        s = total - at if s is None else s
        out.append((at, at + s))
        at += s
    assert at <= total
    return out, at


def run(k, x, sizes):
    """-> (the concatenated steps, how many frames were fed)"""
    pieces, fed = cuts(sizes, x.shape[-1])
    parts = []
    for a, b in pieces:
        y = k.step(x[..., a:b])
        if a == b:
            assert y is None
        else:
            assert tuple(y.shape) == tuple(x.shape[:-1]) + (b - a,)
            parts.append(host(y))
    return np.concatenate(parts, axis=-1), fed


@pytest.mark.parametrize("name", SETS)
@pytest.mark.parametrize("chunking", list(CHUNKINGS))
def test_chunked_steps_are_apply(chunking, name):
    c = Pcen.Config.create(**dict(R.SETS[name], scale=2.0 ** 31))
    x = R.inputs(13, LEAD, BANDS, FRAMES)
    more = R.inputs(14, LEAD, BANDS, 3)[..., 1:]          # two further frames, the first not a row's start
    k = Pcen.Kernel.prepare(c, LEAD, BANDS)
    for dtype, on in ((np.float32, device), (np.float32, np.array), (np.float64, np.array)):
        xs = on(x.astype(dtype))
        for again in (False, True):                       # and again after reset
            k.reset()
            got, fed = run(k, xs, CHUNKINGS[chunking])
            want, zf = Pcen.apply(c, xs[..., :fed], return_state=True)
            what = "%s, %s, %s%s" % (chunking, name, "device" if on is device else np.dtype(dtype).name, ", after reset" if again else "")
            same(got, want, what)
            further = on(more.astype(dtype))
            same(k.step(further), Pcen.apply(c, further, zi=zf), what + ": a further step from the state against apply from zf")
            assert k.flush() == []
    with pytest.raises(Pcen._lib.InvalidArgument):
        k.step(xs[..., :4])                               # drained by the flush
