"""Sequence on MI355X: the pairwise cost matrix of two feature sequences and dynamic time warping (Sakoe & Chiba 1978; Mueller
2007 ch. 4), exported flat as ``cost_matrix`` / ``dtw`` / ``dtw_distance``.  The reference has no such module; the parameters
carry librosa's names.

    cx, cy = chroma_cqt(cc, x), chroma_cqt(cc, y)                          # [...; 12; n] and [...; 12; m], on the device
    C = cost_matrix(cx, cy, metric="cosine")                               # [...; n; m]
    D, path = dtw(cx, cy)                                                  # [...; n; m] and [...; 2; n + m - 1], -1.0 behind the path
    dist = dtw_distance(cx, cy)                                            # [...; 1]: neither D nor the step codes are written
    cells = Sequence.warping_path(path)                                    # int64 [L; 2] per pair on the host (synchronises)

Features are feature-major with frames last, as every feature of this library leaves them; ``X`` and ``Y`` share the leading
axes (the pairs), ``d`` and the dtype.  Float64 inside, one rounding to the dtype of the input.  The recursion is only ``+`` and
``<`` in one stated order (include/soundml_amd.h words the definition), so both kernels, every tiling and a
leading slice of a batch give the same bits.  Device tensors run on the caller's stream and nothing synchronises; device-resident
float64 is refused.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import check, lib
from ._tensor import OUT, STREAM, Batch, prod, refuse_device_float64


def _tile():
    rows, cols = C.c_int64(), C.c_int64()
    check(lib.smx_sequence_tile(C.byref(rows), C.byref(cols)))
    return int(rows.value), int(cols.value)


TILE_ROWS, TILE_COLS = _tile()      # the tile kernel's tile, for shapes on its edges


def _metric(name, metric):
    try:
        return _lib.METRIC[metric]
    except (KeyError, TypeError):
        raise _lib.InvalidArgument("%s: unknown metric %r (one of %s)" % (name, metric, ", ".join(sorted(_lib.METRIC)))) from None


def _weights(name, values, what):
    try:
        w = [float(v) for v in values]
    except TypeError:
        w = []
    if len(w) != 3:
        raise _lib.InvalidArgument("%s: %s holds %d values (one per step: 3)" % (name, what, len(w)))
    return (C.c_double * 3)(*w)


def _pairs(name, X, Y, check_call):
    """(bx, by, lead shape, pairs, d, n, m) once the shapes agree and check_call(d, n, m) has passed, no device touched before"""
    sx, sy = tuple(X.shape), tuple(Y.shape)
    for what, s in (("X", sx), ("Y", sy)):
        if len(s) < 2:
            raise _lib.InvalidArgument("%s: %s has rank %d (features are [...; d; frames]: at least 2)" % (name, what, len(s)))
    if sx[-2] != sy[-2]:
        raise _lib.InvalidArgument("%s: X has %d features and Y has %d (the frames must share d)" % (name, sx[-2], sy[-2]))
    if sx[:-2] != sy[:-2]:
        raise _lib.InvalidArgument("%s: the leading axes of X are %s and those of Y are %s (the pairs must agree)" % (
            name, list(sx[:-2]), list(sy[:-2])))
    d, n, m = int(sx[-2]), int(sx[-1]), int(sy[-1])
    check_call(d, n, m)
    bx, by = Batch(X, name), Batch(Y, name)
    if bx.device != by.device or bx.bytes != by.bytes:
        raise _lib.InvalidArgument("%s: X and Y must share the dtype and lie on the same side (host or device)" % name)
    refuse_device_float64(name, bx, "features are")
    return bx, by, sx[:-2], prod(sx[:-2]), d, n, m


def cost_matrix(X, Y, metric: str = "euclidean"):
    """The pairwise cost of the frames of ``X`` [...; d; n] and ``Y`` [...; d; m] -> [...; n; m] under ``"euclidean"``,
    ``"sqeuclidean"``, ``"cityblock"`` or ``"cosine"``: one ascending chain over the features per cell."""
    name = "cost_matrix"
    k = _metric(name, metric)
    bx, by, lead_shape, pairs, d, n, m = _pairs(name, X, Y, lambda d, n, m: check(lib.smx_cost_matrix_f32(None, None, 0, d, n, m, k, None)))
    return bx.run((lib.smx_cost_matrix_f32, lib.smx_cost_matrix_f64), (bx.ptr(), by.ptr(), pairs, d, n, m, k, OUT),
                  lib.smx_cost_matrix_hbm_f32, (bx.ptr(), by.ptr(), pairs, d, n, m, n, m, k, OUT, STREAM), lead_shape + (n, m),
                  skip=pairs == 0, overwritten=True)


def dtw(X, Y, metric: str = "euclidean", weights_add=(0, 0, 0), weights_mul=(1, 1, 1), subseq: bool = False):
    """Dynamic time warping of ``X`` [...; d; n] against ``Y`` [...; d; m] -> ``(D, path)``: the accumulated cost [...; n; m]
    and the optimal path [...; 2; n + m - 1] in the dtype of the input, row 0 the indices into ``X`` and row 1 those into ``Y``,
    ascending from the path's first cell to its last, ``-1.0`` behind it (``warping_path`` lists the cells).  The steps are
    (1, 1), (0, 1), (1, 0) in this order, step ``s`` costing ``weights_mul[s] * C + weights_add[s]``; a tie keeps the earlier
    step.  ``subseq``: ``X`` may start and end anywhere in ``Y``.  A pair of more than 2^29 cells is refused (``dtw_distance``
    takes it)."""
    name = "dtw"
    k = _metric(name, metric)
    add, mul, sub = _weights(name, weights_add, "weights_add"), _weights(name, weights_mul, "weights_mul"), 1 if subseq else 0
    bx, by, lead_shape, pairs, d, n, m = _pairs(
        name, X, Y, lambda d, n, m: check((lib.smx_dtw_f64 if _wide(X) else lib.smx_dtw_f32)(None, None, 0, d, n, m, k, add, mul, sub, None, None)))
    return bx.run((lib.smx_dtw_f32, lib.smx_dtw_f64), (bx.ptr(), by.ptr(), pairs, d, n, m, k, add, mul, sub, OUT, OUT),
                  lib.smx_dtw_hbm_f32, (bx.ptr(), by.ptr(), pairs, d, n, m, n, m, k, add, mul, sub, OUT, OUT, STREAM),
                  [lead_shape + (n, m), lead_shape + (2, n + m - 1)], skip=pairs == 0, overwritten=(True, False))


def dtw_distance(X, Y, metric: str = "euclidean", weights_add=(0, 0, 0), weights_mul=(1, 1, 1), subseq: bool = False):
    """The total cost of ``dtw`` alone, [...; 1]: the float64 value at the end cell rounded once, i.e. ``D`` at the last cell of
    the path.  Neither ``D`` nor the step codes are written: the face for nearest-neighbour use, without ``dtw``'s size cap."""
    name = "dtw_distance"
    k = _metric(name, metric)
    add, mul, sub = _weights(name, weights_add, "weights_add"), _weights(name, weights_mul, "weights_mul"), 1 if subseq else 0
    bx, by, lead_shape, pairs, d, n, m = _pairs(name, X, Y, lambda d, n, m: check(lib.smx_dtw_distance_f32(None, None, 0, d, n, m, k, add, mul, sub, None)))
    return bx.run((lib.smx_dtw_distance_f32, lib.smx_dtw_distance_f64), (bx.ptr(), by.ptr(), pairs, d, n, m, k, add, mul, sub, OUT),
                  lib.smx_dtw_distance_hbm_f32, (bx.ptr(), by.ptr(), pairs, d, n, m, n, m, k, add, mul, sub, OUT, STREAM), lead_shape + (1,),
                  skip=pairs == 0)


def _wide(x) -> bool:
    """the path of a float64 input holds float64 indices: its size cap is the step codes' alone"""
    return str(getattr(x, "dtype", "")).endswith("float64")


def warping_path(path):
    """The cells of a path [...; 2; n + m - 1] as int64 arrays [L; 2] on the host, (index into X, index into Y) per row: one array
    for a single pair, nested lists of arrays along the leading axes otherwise.  A device path is copied to the host, which
    SYNCHRONISES its stream."""
    a = path.detach().cpu().numpy() if hasattr(path, "detach") else np.asarray(path)

    def walk(p):
        if p.ndim > 2:
            return [walk(q) for q in p]
        return p[:, p[0] >= 0].T.astype(np.int64)
    return walk(a)
