"""cost_matrix / dtw / dtw_distance on the device, BIT FOR BIT against the numpy restatement (tests/sequence_restatement.py: the one
order of DESIGN.md 4.8h, where another order of the feature chain gives other bits, as test_sequence_restatement.py shows).

The shapes (d, n, m) come from the tile kernel's exported tile TR x TC: one cell, one row, one column, a pair under one tile,
(TR - 1, TC + 1), (TR, TC), (TR + 1, 2 TC + 3) -- two by three tiles with short last ones -- and (2 TR + 5, 5): the smallest at
which a lane's strip, the skew, a tile edge, the corner hand-over and a short tile can each go wrong.  Every batch holds a pair as
drawn, one scaled by 1e-6 and one by 1e6.  Faces: host float32, host float64, device float32; the tile route against the general
one (SMX_DISABLE_FAST=1); a leading slice; ties everywhere; one NaN frame.  Two NaNs count as the same bits whatever their payload."""
import contextlib
import functools
import os

import numpy as np
import pytest

import soundml_amd as S
from soundml_amd import Sequence

import sequence_restatement as R

pytestmark = pytest.mark.gpu

TR, TC = Sequence.TILE_ROWS, Sequence.TILE_COLS
GEOMETRIES = R.GEOMETRIES + R.tile_geometries(TR, TC)
MID = (12, 63, 65)
WEIGHTS = [((0, 0, 0), (1, 1, 1)), ((0, 0.5, 0.25), (2, 1, 1))]          # (weights_add, weights_mul)


@contextlib.contextmanager
def general_route():
    """SMX_DISABLE_FAST is read per call"""
    saved = os.environ.get("SMX_DISABLE_FAST")
    os.environ["SMX_DISABLE_FAST"] = "1"
    try:
        yield
    finally:
        if saved is None:
            os.environ.pop("SMX_DISABLE_FAST", None)
        else:
            os.environ["SMX_DISABLE_FAST"] = saved


def device(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()              # a copy: the cached inputs are read-only


def host(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)


def same_bits(got, want, what):
    got, want = host(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, got.dtype, want.shape, want.dtype)
    word = np.int32 if got.dtype == np.float32 else np.int64
    differ = np.ascontiguousarray(got).view(word) != np.ascontiguousarray(want).view(word)
    differ &= ~(np.isnan(got) & np.isnan(want))
    assert not differ.any(), "%s: %d/%d values differ, the first at %s: %r against %r" % (
        what, int(differ.sum()), differ.size, np.argwhere(differ)[0].tolist(), got[differ][0], want[differ][0])


@functools.lru_cache(maxsize=None)
def batch(geometry, dtype, kind="drawn"):
    pair = R.tie_batch(geometry, dtype) if kind == "ties" else R.pair_batch(geometry, dtype)
    if kind == "nan":
        pair[0][0, :, geometry[1] // 2] = np.nan             # one NaN frame in the first pair's X
    for a in pair:
        a.setflags(write=False)
    return pair


@functools.lru_cache(maxsize=None)
def restated(geometry, dtype, metric="euclidean", weights=0, subseq=False, kind="drawn"):
    X, Y = batch(geometry, dtype, kind)
    out = R.dtw(X, Y, metric, WEIGHTS[weights][0], WEIGHTS[weights][1], subseq)
    for a in out:
        a.setflags(write=False)
    return out


def faces(geometry, kind="drawn"):
    x32, y32 = batch(geometry, np.float32, kind)
    return [("host float32", np.float32, x32, y32), ("host float64", np.float64) + batch(geometry, np.float64, kind),
            ("device float32", np.float32, device(x32), device(y32))]


def check_dtw(geometry, metric, weights, subseq, kind="drawn", routes=False):
    d, n, m = geometry
    add, mul = WEIGHTS[weights]
    for what, dtype, x, y in faces(geometry, kind):
        D, path, dist = restated(geometry, dtype, metric, weights, subseq, kind)
        assert D.shape == (3, n, m) and path.shape == (3, 2, n + m - 1) and dist.shape == (3, 1)
        for route in ((contextlib.nullcontext, ""), (general_route, ", general route")) if routes else ((contextlib.nullcontext, ""),):
            with route[0]():
                gD, gpath = S.dtw(x, y, metric=metric, weights_add=add, weights_mul=mul, subseq=subseq)
                gdist = S.dtw_distance(x, y, metric=metric, weights_add=add, weights_mul=mul, subseq=subseq)
            tag = "%s%s, %s, weights %d, subseq %s" % (what, route[1], metric, weights, subseq)
            same_bits(gD, D, tag + ": D")
            same_bits(gpath, path, tag + ": path")
            same_bits(gdist, dist, tag + ": distance")
            # the distance is D at the path's last cell, face by face
            hD, hp = host(gD), host(gpath)
            for p in range(3):
                L = int((hp[p, 0] >= 0).sum())
                same_bits(host(gdist)[p, 0], hD[p, int(hp[p, 0, L - 1]), int(hp[p, 1, L - 1])], tag + ": distance against D")


@pytest.mark.parametrize("subseq", [False, True])
@pytest.mark.parametrize("weights", [0, 1])
@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_dtw_bit_for_bit_against_the_restatement(geometry, weights, subseq):
    check_dtw(geometry, "euclidean", weights, subseq)


@pytest.mark.parametrize("metric", R.METRICS)
def test_metrics(metric):
    for what, dtype, x, y in faces(MID):
        X, Y = batch(MID, dtype)
        want = R.cost_matrix(X, Y, metric)
        same_bits(S.cost_matrix(x, y, metric=metric), want, "%s, %s" % (what, metric))
        with general_route():
            same_bits(S.cost_matrix(x, y, metric=metric), want, "%s, %s, general route" % (what, metric))
    check_dtw(MID, metric, 1, True)


@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_cost_matrix(geometry):
    for what, dtype, x, y in faces(geometry):
        X, Y = batch(geometry, dtype)
        same_bits(S.cost_matrix(x, y), R.cost_matrix(X, Y), what)


@pytest.mark.parametrize("geometry", [MID, (13, TR + 1, 2 * TC + 3)])
def test_ties(geometry):
    """features from {0, 1, 2} with d = 2: ties everywhere, and the path is still the restatement's: the strict-less rule and the
    step order"""
    geometry = (2,) + geometry[1:]
    for subseq in (False, True):
        check_dtw(geometry, "sqeuclidean", 0, subseq, kind="ties", routes=True)


@pytest.mark.parametrize("geometry", [MID, (12, TR - 1, TC + 1), (13, TR + 1, 2 * TC + 3), (2, 2 * TR + 5, 5)])
def test_routes_and_slices(geometry):
    x, y = (device(a) for a in batch(geometry, np.float32))
    for subseq in (False, True):
        D, path = S.dtw(x, y, subseq=subseq)
        dist = S.dtw_distance(x, y, subseq=subseq)
        with general_route():
            gD, gpath = S.dtw(x, y, subseq=subseq)
            gdist = S.dtw_distance(x, y, subseq=subseq)
        same_bits(gD, host(D), "general route: D")
        same_bits(gpath, host(path), "general route: path")
        same_bits(gdist, host(dist), "general route: distance")
        sD, spath = S.dtw(x[:2], y[:2], subseq=subseq)
        same_bits(sD, host(D)[:2], "a leading slice: D")
        same_bits(spath, host(path)[:2], "a leading slice: path")
        same_bits(S.dtw_distance(x[:1], y[:1], subseq=subseq), host(dist)[:1], "a leading slice: distance")
    same_bits(S.cost_matrix(x[:2], y[:2]), host(S.cost_matrix(x, y))[:2], "a leading slice: cost")


@pytest.mark.parametrize("geometry", [MID, (13, TR + 1, 2 * TC + 3)])
def test_nan_frame(geometry):
    """one NaN frame in X: the restatement's NaN footprint in D, bit for bit, on every face and both routes"""
    D = restated(geometry, np.float32, kind="nan")[0]
    at = geometry[1] // 2
    assert np.isnan(D[0, at:]).all() and not np.isnan(D[0, :at]).any() and not np.isnan(D[1:]).any()
    for subseq in (False, True):
        check_dtw(geometry, "euclidean", 0, subseq, kind="nan", routes=True)


def test_leading_axes_and_empty_batches():
    x, y = batch(MID, np.float32)
    X, Y = device(np.stack([x, x])[:, :2]), device(np.stack([y, y])[:, :2])     # [2; 2; d; .]
    D, path = S.dtw(X, Y)
    assert tuple(D.shape) == (2, 2, 63, 65) and tuple(path.shape) == (2, 2, 2, 127)
    same_bits(D[1], restated(MID, np.float32)[0][:2], "two leading axes")
    cells = Sequence.warping_path(path)
    assert len(cells) == 2 and len(cells[0]) == 2 and cells[0][0].dtype == np.int64 and cells[0][0][0].tolist() == [0, 0]
    assert cells[1][1][-1].tolist() == [62, 64]
    e = S.dtw(X[:0], Y[:0])
    assert tuple(e[0].shape) == (0, 2, 63, 65) and tuple(e[1].shape) == (0, 2, 2, 127) and e[0].is_cuda
    assert tuple(S.dtw_distance(X[:0], Y[:0]).shape) == (0, 2, 1) and tuple(S.cost_matrix(X[:0], Y[:0]).shape) == (0, 2, 63, 65)
    with pytest.raises(S.Failure, match="device-resident float64"):
        S.dtw(X.double(), Y.double())
