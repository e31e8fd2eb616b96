"""Decompose restated in numpy, every chain explicit: vectorised over the cells and looped over the summed index, in the order
include/soundml_amd.h and DESIGN.md 4.8i state.

dtype float64: the formulas in float64 (a product and a sum round one after the other; the library's float64 faces fuse them,
which its 1e-13 bound covers).  dtype float32: the library's float32 interior literally, fmaf emulated as the float64 product and
sum rounded to float32 (the product of two float32 values is exact in float64).

  over f or t   32-block after 32-block, inside a block position i = 2 r + h is offset (r & 3) + 8 (r >> 2) + 4 h; the last block
                is padded to 32 with terms fma(0, 0, acc)
  over k        ascending, padded to an even count with one term fma(0, 0, acc)
"""
import numpy as np

EPS = 2.0 ** -23
FROBENIUS, KL = "frobenius", "kullback-leibler"
SNAPSHOTS = (0, 1, 2, 8, 200)


def perm32(i):
    r, h = i >> 1, i & 1
    return (r & 3) + 8 * (r >> 2) + 4 * h


def order32(n):
    """the summed index at every step of a chain over n; -1: a pad term"""
    steps = []
    for b in range(0, n, 32):
        for i in range(32):
            idx = b + perm32(i)
            steps.append(idx if idx < n else -1)
    return steps


def order_k(K):
    return list(range(K)) + ([-1] if K & 1 else [])


class Chain:
    """acc = fma(a, b, acc) over the cells of one shape, from 0.0"""

    def __init__(self, shape, dtype):
        self.dtype = np.dtype(dtype)
        self.acc = np.zeros(shape, np.float64)
        self.tmp = np.empty(shape, np.float64)
        self.narrow = np.empty(shape, np.float32) if self.dtype == np.float32 else None

    def step(self, a, b):
        np.multiply(a, b, out=self.tmp)
        np.add(self.tmp, self.acc, out=self.acc)
        if self.narrow is not None:
            self.narrow[...] = self.acc
            self.acc[...] = self.narrow

    def pad(self):
        self.acc += 0.0             # fma(0, 0, acc): only a zero's sign can change

    def value(self):
        return self.acc.astype(self.dtype)


def inner_f(W, S, dtype):
    """[...; F; K] and [...; F; N] -> [...; K; N]: sum over f of W[f, k] S[f, n]"""
    W64, S64 = W.astype(np.float64), S.astype(np.float64)
    c = Chain(W.shape[:-2] + (W.shape[-1], S.shape[-1]), dtype)
    for f in order32(W.shape[-2]):
        if f < 0:
            c.pad()
        else:
            c.step(W64[..., f, :, None], S64[..., f, None, :])
    return c.value()


def inner_t(S, H, dtype):
    """[...; M; T] and [...; K; T] -> [...; M; K]: sum over t of S[m, t] H[k, t]"""
    S64, H64 = S.astype(np.float64), H.astype(np.float64)
    c = Chain(S.shape[:-1] + (H.shape[-2],), dtype)
    for t in order32(S.shape[-1]):
        if t < 0:
            c.pad()
        else:
            c.step(S64[..., :, t, None], H64[..., None, :, t])
    return c.value()


def inner_k(A, B, dtype, keep=None):
    """[...; M; K] and [...; K; N] -> [...; M; N], ascending over k; a component outside `keep` enters as fma(0, 0, acc)"""
    A64, B64 = A.astype(np.float64), B.astype(np.float64)
    c = Chain(A.shape[:-1] + (B.shape[-1],), dtype)
    for k in order_k(A.shape[-1]):
        if k < 0 or (keep is not None and k not in keep):
            c.pad()
        else:
            c.step(A64[..., :, k, None], B64[..., None, k, :])
    return c.value()


def floor(x, dtype):
    eps = np.dtype(dtype).type(EPS)
    return np.where(x < eps, eps, x)            # a NaN stays a NaN


def update_h(V, W, H, beta, dtype):
    if beta == FROBENIUS:
        num, den = inner_f(W, V, dtype), inner_k(inner_f(W, W, dtype), H, dtype)
    else:
        R = V / floor(inner_k(W, H, dtype), dtype)
        num, den = inner_f(W, R, dtype), inner_f(W, np.ones(W.shape[:-1] + (1,), dtype), dtype)          # [...; K; 1]
    return (H * num) / floor(den, dtype)


def update_w(V, W, H, beta, dtype):
    if beta == FROBENIUS:
        G = inner_t(H, H, dtype)                                             # [...; K; K], symmetric in its bits
        num, den = inner_t(V, H, dtype), inner_k(W, G, dtype)
    else:
        R = V / floor(inner_k(W, H, dtype), dtype)
        num, den = inner_t(R, H, dtype), inner_t(np.ones(H.shape[:-2] + (1, H.shape[-1]), dtype), H, dtype)   # [...; 1; K]
    return (W * num) / floor(den, dtype)


def nmf(V, W0, H0, n_iter, beta, dtype, snapshots=()):
    """(W, H) after n_iter rounds, or {round: (W, H)} for the rounds in `snapshots`"""
    V, W, H = V.astype(dtype), W0.astype(dtype), H0.astype(dtype)
    out = {0: (W.copy(), H.copy())} if 0 in snapshots else {}
    with np.errstate(all="ignore"):
        for r in range(1, n_iter + 1):
            H = update_h(V, W, H, beta, dtype)
            W = update_w(V, W, H, beta, dtype)
            if r in snapshots:
                out[r] = (W.copy(), H.copy())
    return out if snapshots else (W, H)


def activations(V, W, H0, n_iter, beta, dtype):
    V, W, H = V.astype(dtype), W.astype(dtype), H0.astype(dtype)
    with np.errstate(all="ignore"):
        for _ in range(n_iter):
            H = update_h(V, W, H, beta, dtype)
    return H


def reconstruct(W, H, components=None, as_mask=False):
    dtype = H.dtype
    keep = None if components is None else set(int(k) for k in components)
    x = inner_k(W, H, dtype, keep)
    if not as_mask:
        return x
    with np.errstate(all="ignore"):
        return x / floor(inner_k(W, H, dtype), dtype)


def divergence(V, W, H, beta, parts=False):
    """[...; 1] in the dtype of V: float64 inside, X = W H an ascending chain over k, the sums ascending over t per row and then
    ascending over the rows.  parts: also sum |term| of the KL sums, the scale of its tolerance"""
    dtype = V.dtype
    V64, W64, H64 = V.astype(np.float64), W.astype(np.float64), H.astype(np.float64)
    X = np.zeros(V.shape, np.float64)
    for k in range(W.shape[-1]):
        X = X + W64[..., :, k, None] * H64[..., None, k, :]
    rows = np.zeros((3,) + V.shape[:-1], np.float64)
    scale = np.zeros(V.shape[:-1], np.float64)
    with np.errstate(all="ignore"):
        for t in range(V.shape[-1]):
            v, x = V64[..., t], X[..., t]
            if beta == FROBENIUS:
                d = v - x
                rows[0] = rows[0] + d * d
                rows[1] = rows[1] + v * v
            else:
                term = v * np.log(v / x)
                rows[0] = np.where(v > 0, rows[0] + term, rows[0])
                rows[1] = rows[1] + v
                rows[2] = rows[2] + x
                scale = scale + np.where(v > 0, np.abs(term), 0.0) + np.abs(v) + np.abs(x)
        total = np.zeros((3,) + V.shape[:-2], np.float64)
        for f in range(V.shape[-2]):
            total = total + rows[..., f]
        if beta == FROBENIUS:
            out = np.sqrt(total[0] / total[1])
        else:
            out = ((total[0] - total[1]) + total[2]) / total[1]
    out = out.astype(dtype)[..., None]
    return (out, (scale.sum(-1) / total[1])[..., None]) if parts else out


def initial(lead, F, T, K, seed=0):
    lead = tuple(lead)
    W0 = 1.0 - np.random.Generator(np.random.PCG64([seed, 0])).random(lead + (F, K))
    H0 = 1.0 - np.random.Generator(np.random.PCG64([seed, 1])).random(lead + (K, T))
    return W0, H0


def problem(geometry, clips=4, seed=11, rank=None):
    """V = W* H* + 0.01 u rounded to float32, [clips; F; T]: `clips` clips drawn in C order, so fewer clips are a leading slice"""
    F, T, K = geometry
    rank = max(1, min(K, 8)) if rank is None else rank
    rng = np.random.Generator(np.random.PCG64([seed, F, T, K]))
    V = np.empty((clips, F, T), np.float32)
    for c in range(clips):
        Wt, Ht = rng.random((F, rank)) ** 3, rng.random((rank, T)) ** 2
        V[c] = (Wt @ Ht + 0.01 * rng.random((F, T))).astype(np.float32)
    return V
