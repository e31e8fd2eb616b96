"""numpy restatement of Iir (include/soundml_amd.h words the definition, DESIGN.md 4.8k the order), no GPU.  Every product and every
sum is its own numpy operation on float64 arrays, so nothing fuses; channels are vectorised, time is a Python loop.

    serial(sos, x, zi)              the cascade sample by sample: scipy.signal.sosfilt's float64 output
    stated(sos, x, zi, block)       the library's order: blocks of `block` samples, s_{b+1} = M s_b + w_b (ascending j, w last)
    filtfilt(sos, x, block)         sosfiltfilt with its defaults by two such passes (block None: two serial passes)
    Kernel(sos, channels, block)    the streaming form, sample by sample with a carried position (the second, independent walk)
States are [channels; S; 2]; flat index 2 k + r is z[k][r]."""
import functools

import numpy as np

BLOCK = 256
SPAN_BLOCKS = 64
MAX_SECTIONS = 8


def _sos(sos):
    sos = np.asarray(sos, np.float64)
    assert sos.ndim == 2 and sos.shape[1] == 6 and np.all(sos[:, 3] == 1.0)
    return sos


def step(sos, u, z):
    """one sample u [C] through the cascade, the states z [C; S; 2] updated in place -> y [C]"""
    for k in range(sos.shape[0]):
        b0, b1, b2, _, a1, a2 = sos[k]
        y = b0 * u + z[:, k, 0]
        z[:, k, 0] = (b1 * u - a1 * y) + z[:, k, 1]
        z[:, k, 1] = b2 * u - a2 * y
        u = y
    return u


def _start(sos, channels, zi):
    z = np.zeros((channels, sos.shape[0], 2))
    if zi is not None:
        z[:] = np.asarray(zi, np.float64)
    return z


def serial(sos, x, zi=None, return_state=False):
    sos = _sos(sos)
    x = np.atleast_2d(np.asarray(x, np.float64))
    z = _start(sos, x.shape[0], zi)
    y = np.empty_like(x)
    for t in range(x.shape[1]):
        y[:, t] = step(sos, x[:, t], z)
    return (y, z) if return_state else y


def matrix(sos, block=BLOCK):
    """M [2S; 2S]: column i is the end state of `block` zero-input steps from the unit state e_i"""
    sos = _sos(sos)
    n = 2 * sos.shape[0]
    z = np.eye(n).reshape(n, sos.shape[0], 2)           # channel i starts from e_i
    zero = np.zeros(n)
    for _ in range(block):
        step(sos, zero, z)
    return np.ascontiguousarray(z.reshape(n, n).T)


def advance(M, s, w):
    """s_{b+1}[i] = (((M[i][0] s[0] + M[i][1] s[1]) + ...) + M[i][2S-1] s[2S-1]) + w[i] per channel; s, w [C; 2S]"""
    acc = M[None, :, 0] * s[:, None, 0]
    for j in range(1, M.shape[1]):
        acc = acc + M[None, :, j] * s[:, None, j]
    return acc + w


def stated(sos, x, zi=None, block=BLOCK, return_state=False):
    """the whole blocks of every channel side by side (a block is a row: `block` time steps in all), as the library's block
    route walks them: w_b from zero, the chain s_{b+1} = M s_b + w_b, the outputs of block b from s_b; then the tail serially"""
    sos = _sos(sos)
    x = np.atleast_2d(np.asarray(x, np.float64))
    C, n = x.shape
    S = sos.shape[0]
    nb = n // block
    s = _start(sos, C, zi)
    y = np.empty_like(x)
    if nb:
        M = matrix(sos, block)
        xb = x[:, :nb * block].reshape(C * nb, block)
        w = np.zeros((C * nb, S, 2))
        for t in range(block):
            step(sos, xb[:, t], w)
        w = w.reshape(C, nb, 2 * S)
        entering = np.empty((C, nb, 2 * S))
        cur = s.reshape(C, 2 * S)
        for b in range(nb):
            entering[:, b] = cur
            cur = advance(M, cur, w[:, b])
        z = entering.reshape(C * nb, S, 2).copy()
        yb = np.empty((C * nb, block))
        for t in range(block):
            yb[:, t] = step(sos, xb[:, t], z)
        y[:, :nb * block] = yb.reshape(C, nb * block)
        s = cur.reshape(C, S, 2)
    run = s.copy()
    for t in range(nb * block, n):
        y[:, t] = step(sos, x[:, t], run)
    return (y, run) if return_state else y


def zi(sos):
    """the unit-step steady state in closed form, [S; 2]"""
    sos = _sos(sos)
    out = np.zeros((sos.shape[0], 2))
    scale = 1.0
    for k in range(sos.shape[0]):
        b0, b1, b2, _, a1, a2 = sos[k]
        den = (1.0 + a1) + a2
        assert den != 0.0
        g = ((b0 + b1) + b2) / den
        out[k, 0] = scale * (g - b0)
        out[k, 1] = scale * (b2 - a2 * g)
        scale = scale * g
    return out


def padlen(sos):
    sos = _sos(sos)
    return 3 * (2 * sos.shape[0] + 1 - min(int((sos[:, 2] == 0).sum()), int((sos[:, 5] == 0).sum())))


def odd_extension(x, p):
    """2 x[0] - x[p], ..., 2 x[0] - x[1] | x | 2 x[n-1] - x[n-2], ..., 2 x[n-1] - x[n-1-p], in float64"""
    x = np.atleast_2d(np.asarray(x, np.float64))
    assert x.shape[1] > p
    return np.concatenate([2.0 * x[:, :1] - x[:, p:0:-1], x, 2.0 * x[:, -1:] - x[:, -2:-(p + 2):-1]], axis=1)


def filtfilt(sos, x, block=BLOCK):
    """float64 [C; n]; block None: both passes serial"""
    sos = _sos(sos)
    p = padlen(sos)
    ext = odd_extension(x, p)
    z = zi(sos)
    run = serial if block is None else functools.partial(stated, block=block)
    fwd = run(sos, ext, z[None] * ext[:, 0, None, None])
    back = np.ascontiguousarray(fwd[:, ::-1])
    out = run(sos, back, z[None] * back[:, 0, None, None])
    return np.ascontiguousarray(out[:, ::-1][:, p:ext.shape[1] - p])


class Kernel:
    """sample by sample: the state entering the block, the partial zero-state run, the running state, the position"""

    def __init__(self, sos, channels, block=BLOCK):
        self.sos, self.C, self.block = _sos(sos), int(channels), int(block)
        self.M = matrix(self.sos, self.block)
        self.reset()

    def reset(self):
        S = self.sos.shape[0]
        self.s = np.zeros((self.C, S, 2))
        self.w = np.zeros((self.C, S, 2))
        self.r = np.zeros((self.C, S, 2))
        self.pos = 0
        self.drained = False

    def step(self, chunk):
        assert not self.drained
        chunk = np.atleast_2d(np.asarray(chunk, np.float64))
        if chunk.shape[1] == 0:
            return None
        S = self.sos.shape[0]
        y = np.empty_like(chunk)
        for t in range(chunk.shape[1]):
            y[:, t] = step(self.sos, chunk[:, t], self.r)
            step(self.sos, chunk[:, t], self.w)
            self.pos += 1
            if self.pos == self.block:
                self.s = advance(self.M, self.s.reshape(self.C, 2 * S), self.w.reshape(self.C, 2 * S)).reshape(self.C, S, 2)
                self.r = self.s.copy()
                self.w = np.zeros_like(self.s)
                self.pos = 0
        return y

    def flush(self):
        self.drained = True
        return []


# ---- the shared cases of the GPU tests ---------------------------------------------------------------------------------------

# stable sections written out (no designer at test time): a Butterworth 2 low-pass at 0.1, a high-pass at 20 Hz / 48 kHz, and the
# two K-weighting biquads of BS.1770 at 48 kHz; longer cascades repeat them in turn
SECTIONS = np.array([
    [0.02008336556421123, 0.04016673112842246, 0.02008336556421123, 1.0, -1.5610180758007182, 0.6413515380575631],
    [0.9981505111904518, -1.9963010223809037, 0.9981505111904518, 1.0, -1.996297601769122, 0.9963044429926857],
    [1.53512485958697, -2.69169618940638, 1.19839281085285, 1.0, -1.69065929318241, 0.73248077421585],
    [1.0, -2.0, 1.0, 1.0, -1.99004745483398, 0.99007225036621],
])


def cascade(S):
    return np.ascontiguousarray(SECTIONS[np.arange(S) % len(SECTIONS)])


@functools.lru_cache(maxsize=None)
def batch(seed, channels, n):
    """float32 [channels; n]: channels as drawn, scaled by 1e-6 and by 1e6 in turn"""
    x = np.random.default_rng(seed).uniform(-1, 1, size=(channels, n))
    x = (x * np.array([1.0, 1e-6, 1e6])[np.arange(channels) % 3, None]).astype(np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def batch_state(seed, channels, S):
    z = np.random.default_rng(seed).uniform(-1, 1, size=(channels, S, 2))
    z.setflags(write=False)
    return z


@functools.lru_cache(maxsize=None)
def expected(S, seed, channels, n, zi_kind=None):
    """(y float64 [channels; n], zf) of the stated order; zi_kind None | "call" | "rows" """
    z = None if zi_kind is None else batch_state(seed + 1, 1, S)[0] if zi_kind == "call" else batch_state(seed + 1, channels, S)
    y, zf = stated(cascade(S), batch(seed, channels, n), z, return_state=True)
    y.setflags(write=False)
    zf.setflags(write=False)
    return y, zf


@functools.lru_cache(maxsize=None)
def expected_filtfilt(S, seed, channels, n):
    y = filtfilt(cascade(S), batch(seed, channels, n))
    y.setflags(write=False)
    return y
