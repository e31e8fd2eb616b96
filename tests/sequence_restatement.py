"""numpy restatement of Sequence (include/soundml_amd.h words the definition, DESIGN.md 4.8h the orders), no GPU.  Every add is
explicit: the feature loop is a Python loop over k, so nothing is left to numpy's pairwise sums, and numpy never fuses a product
with a sum.  The recursion is only + and < on the same operands, so sweeping a whole anti-diagonal at once gives the bits of any
other order of visiting the cells."""
import numpy as np

METRICS = ("euclidean", "sqeuclidean", "cityblock", "cosine")
# (d, n, m): one cell, one row, one column, and a pair under one tile; the GPU tests add the shapes on the tile kernel's edges
GEOMETRIES = [(1, 1, 1), (3, 1, 7), (3, 7, 1), (12, 63, 65)]


def tile_geometries(TR, TC):
    """the shapes at which a lane's strip, the skew, a tile edge, the corner hand-over and a short tile can each go wrong"""
    return [(12, TR - 1, TC + 1), (12, TR, TC), (13, TR + 1, 2 * TC + 3), (2, 2 * TR + 5, 5)]


def pair_batch(geometry, dtype=np.float32):
    """(X [3; d; n], Y [3; d; m]): a pair as drawn (uniform in [0, 1), as chroma is), one scaled by 1e-6 and one by 1e6"""
    d, n, m = geometry
    rng = np.random.default_rng(100000 * d + 1000 * n + m)
    x, y = rng.random((3, d, n)), rng.random((3, d, m))
    for a in (x, y):
        a[1] *= 1e-6
        a[2] *= 1e6
    return x.astype(np.float32).astype(dtype), y.astype(np.float32).astype(dtype)


def tie_batch(geometry, dtype=np.float32):
    """features drawn from {0, 1, 2}: ties everywhere"""
    d, n, m = geometry
    rng = np.random.default_rng(7 + 100000 * d + 1000 * n + m)
    return rng.integers(0, 3, (3, d, n)).astype(dtype), rng.integers(0, 3, (3, d, m)).astype(dtype)


# ---- the cost ----------------------------------------------------------------------------------------------------------------------

def cost_wide(X, Y, metric="euclidean", descending=False):
    """C [...; n; m] in float64, before the rounding: one chain over k from 0.0 per cell, ascending (descending: the other order,
    which test_sequence_restatement.py shows to give other bits)"""
    X, Y = np.asarray(X, np.float64), np.asarray(Y, np.float64)
    d = X.shape[-2]
    shape = X.shape[:-2] + (X.shape[-1], Y.shape[-1])
    a, xx, yy = np.zeros(shape), np.zeros(shape), np.zeros(shape)
    with np.errstate(all="ignore"):
        for k in (range(d - 1, -1, -1) if descending else range(d)):
            x, y = X[..., k, :, None], Y[..., k, None, :]
            if metric == "cosine":
                a = a + x * y
                xx = xx + x * x                    # (a function of the row alone, broadcast over the columns)
                yy = yy + y * y
            elif metric == "cityblock":
                a = a + np.abs(x - y)
            else:
                diff = x - y
                a = a + diff * diff
        if metric == "cosine":
            return 1.0 - a / (np.sqrt(xx) * np.sqrt(yy))
        return np.sqrt(a) if metric == "euclidean" else a


def cost_matrix(X, Y, metric="euclidean"):
    return cost_wide(X, Y, metric).astype(np.asarray(X).dtype)


# ---- the recursion -----------------------------------------------------------------------------------------------------------------

def accumulate(C, weights_add=(0, 0, 0), weights_mul=(1, 1, 1), subseq=False):
    """(D, steps) of a float64 cost [...; n; m]: D in float64 and the step code of every cell, one anti-diagonal at a time"""
    C = np.asarray(C, np.float64)
    n, m = C.shape[-2:]
    wa, wm = [np.float64(v) for v in weights_add], [np.float64(v) for v in weights_mul]
    D, S = np.zeros(C.shape), np.zeros(C.shape, np.int8)
    with np.errstate(all="ignore"):
        for g in range(n + m - 1):
            i = np.arange(max(0, g - m + 1), min(n - 1, g) + 1)
            j = g - i
            hi, hj = i > 0, j > 0
            im, jm = np.maximum(i - 1, 0), np.maximum(j - 1, 0)
            c = C[..., i, j]
            c0 = (D[..., im, jm] + wm[0] * c) + wa[0]
            c1 = (D[..., i, jm] + wm[1] * c) + wa[1]
            c2 = (D[..., im, j] + wm[2] * c) + wa[2]
            have = np.broadcast_to(hi & hj, c.shape)
            best, code = c0, np.zeros(c.shape, np.int8)
            take = hj & (~have | (c1 < best))
            best, code, have = np.where(take, c1, best), np.where(take, 1, code), have | hj
            take = hi & (~have | (c2 < best))
            best, code = np.where(take, c2, best), np.where(take, 2, code)
            start = ~hi & (~hj | bool(subseq))
            best, code = np.where(start, c, best), np.where(start, 1, code)
            D[..., i, j] = best
            S[..., i, j] = code
    return D, S


def end_column(row, subseq):
    """the end cell's column: m - 1, or with subseq the sequential rule over row n - 1 (start from 0, replace only if strictly
    smaller)"""
    if not subseq:
        return len(row) - 1
    best, at = row[0], 0
    for j in range(1, len(row)):
        if row[j] < best:
            best, at = row[j], j
    return at


def backtrack(S, jend, subseq):
    """the cells from the path's first to its last, [L; 2], following the step codes of one pair back from (n - 1, jend)"""
    i, j = S.shape[0] - 1, jend
    cells = [(i, j)]
    while not (i == 0 and (j == 0 or subseq)):
        s = 1 if i == 0 else 2 if j == 0 else int(S[i, j])
        i, j = (i - 1, j - 1) if s == 0 else (i, j - 1) if s == 1 else (i - 1, j)
        cells.append((i, j))
    return np.array(cells[::-1], np.int64)


def path_rows(cells, n, m, dtype):
    """[2; n + m - 1] in dtype: the indices into X, then those into Y, -1.0 behind the path"""
    out = np.full((2, n + m - 1), -1.0, dtype)
    out[:, :len(cells)] = cells.T
    return out


def dtw(X, Y, metric="euclidean", weights_add=(0, 0, 0), weights_mul=(1, 1, 1), subseq=False):
    """(D [...; n; m], path [...; 2; n + m - 1], distance [...; 1]) in the dtype of X"""
    X = np.asarray(X)
    dtype, lead = X.dtype, X.shape[:-2]
    n, m = X.shape[-1], np.asarray(Y).shape[-1]
    D, S = accumulate(cost_wide(X, Y, metric), weights_add, weights_mul, subseq)
    path, dist = np.empty(lead + (2, n + m - 1), dtype), np.empty(lead + (1,), dtype)
    for at in np.ndindex(*lead):
        jend = end_column(D[at][n - 1], subseq)
        path[at] = path_rows(backtrack(S[at], jend, subseq), n, m, dtype)
        dist[at] = D[at][n - 1, jend]
    return D.astype(dtype), path, dist
