"""numpy restatements of the energy features (energy.ml), no GPU.

Two forms of each audio feature:
  * reference order: explicitly padded frames, np.mean / np.sum in float64 -- what energy.ml writes;
  * kernel order: the one summation order of DESIGN.md 4.8e, every add explicit (nothing is left to np.sum's pairwise tree):
      1. a frame is cut into consecutive blocks of min(hop, frame_length) samples from its start, the last may be short;
      2. in a block lane l of 64 adds the squares of elements l, l + 64, ... in ascending order; the 64 lane sums meet in the
         butterfly v[l] += v[l ^ d] for d = 32, 16, 8, 4, 2, 1;
      3. the frame's sum is the first block's partial, the others added to it in ascending order.
    Lanes without an element hold 0.0, and x + 0.0 == x bit for bit for every sum of squares, so a block is padded with zeros
    to a multiple of 64 here.
"""
import numpy as np

SEED = 20260812
LANES = 64
XOR_DISTANCES = (32, 16, 8, 4, 2, 1)


def lcg_values(count, seed=SEED):
    """energy_goldens.ml:25-29: the 31-bit LCG, state / 2^30 - 1"""
    out = np.empty(count, np.float64)
    state = seed
    for i in range(count):
        state = (1103515245 * state + 12345) % (1 << 31)
        out[i] = state / float(1 << 30) - 1.0
    return out


def frames(n, frame_length, hop):
    """energy.ml:114-118"""
    if n == 0:
        return 0
    padded = n + 2 * (frame_length // 2)
    return 0 if padded < frame_length else 1 + (padded - frame_length) // hop


def padded_frames(x, frame_length, hop, mode):
    """[...; n] -> float64 [...; count; frame_length]: the frames of the explicitly padded signal"""
    x = np.asarray(x)
    border = frame_length // 2
    width = [(0, 0)] * (x.ndim - 1) + [(border, border)]
    p = np.pad(x, width, mode=mode) if x.shape[-1] else x
    count = frames(x.shape[-1], frame_length, hop)
    index = np.arange(count)[:, None] * hop + np.arange(frame_length)[None, :]
    return p[..., index].astype(np.float64)


def segment_frames(x, frame_length, hop, count):
    """the uncentred frames [0, count) of a segment"""
    index = np.arange(count)[:, None] * hop + np.arange(frame_length)[None, :]
    return np.asarray(x)[..., index].astype(np.float64)


# ---- reference order ---------------------------------------------------------------------------------------------------------

def rms_reference(x, frame_length=2048, hop=512):
    f = padded_frames(x, frame_length, hop, "constant")
    return np.sqrt(np.mean(np.square(f), axis=-1))[..., None, :].astype(np.asarray(x).dtype)


def crossings_reference(f, frame_length, threshold):
    negative = f < -threshold
    changes = negative[..., 1:] != negative[..., :-1]
    return np.sum(changes.astype(np.float64), axis=-1) / float(frame_length)


def zcr_reference(x, frame_length=2048, hop=512, threshold=1e-10):
    f = padded_frames(x, frame_length, hop, "edge")
    return crossings_reference(f, frame_length, threshold)[..., None, :].astype(np.asarray(x).dtype)


def spectrogram_weights(frame_length):
    w = np.ones(frame_length // 2 + 1)
    w[0] = 0.5
    if frame_length % 2 == 0:
        w[-1] = 0.5
    return w


def rms_of_spectrogram_reference(s, frame_length=2048):
    s = np.asarray(s)
    w = spectrogram_weights(frame_length)[:, None]
    power = np.sum(np.square(s.astype(np.float64)) * w, axis=-2, keepdims=True)
    power = (power * 2.0) / (float(frame_length) * float(frame_length))
    return np.sqrt(power).astype(s.dtype)


# ---- kernel order ------------------------------------------------------------------------------------------------------------

def block_partial(squares):
    """float64 [...; len] -> [...]: step 2 of the order"""
    length = squares.shape[-1]
    rows = -(-length // LANES)
    padded = np.zeros(squares.shape[:-1] + (rows * LANES,), np.float64)
    padded[..., :length] = squares
    lanes = padded.reshape(squares.shape[:-1] + (rows, LANES))
    acc = lanes[..., 0, :].copy()
    for r in range(1, rows):
        acc = acc + lanes[..., r, :]
    for d in XOR_DISTANCES:
        acc = acc[..., :d] + acc[..., d:2 * d]
    return acc[..., 0]


def sum_of_squares_kernel_order(f, hop):
    """float64 frames [...; count; frame_length] -> [...; count]"""
    frame_length = f.shape[-1]
    blk = min(hop, frame_length)
    squares = np.square(f)
    total = None
    for b0 in range(0, frame_length, blk):
        part = block_partial(squares[..., b0:min(b0 + blk, frame_length)])
        total = part if total is None else total + part
    return total


def rms_kernel_order_of_frames(f, hop, dtype):
    return np.sqrt(sum_of_squares_kernel_order(f, hop) / float(f.shape[-1]))[..., None, :].astype(dtype)


def rms_kernel_order(x, frame_length=2048, hop=512):
    return rms_kernel_order_of_frames(padded_frames(x, frame_length, hop, "constant"), hop, np.asarray(x).dtype)


def zcr_kernel_order_of_frames(f, hop, threshold, dtype):
    """counts inside each block, the crossings at the joins of a frame's blocks, none at the frame's first position"""
    frame_length = f.shape[-1]
    blk = min(hop, frame_length)
    negative = f < -threshold
    count = np.zeros(f.shape[:-1], np.int64)
    for b0 in range(0, frame_length, blk):
        block = negative[..., b0:min(b0 + blk, frame_length)]
        count += np.sum(block[..., 1:] != block[..., :-1], axis=-1)
        if b0 > 0:
            count += negative[..., b0] != negative[..., b0 - 1]
    return (count.astype(np.float64) / float(frame_length))[..., None, :].astype(dtype)


def zcr_kernel_order(x, frame_length=2048, hop=512, threshold=1e-10):
    return zcr_kernel_order_of_frames(padded_frames(x, frame_length, hop, "edge"), hop, threshold, np.asarray(x).dtype)


def rms_of_spectrogram_ordered(s, frame_length=2048):
    """the bins walked in ascending order, one add each"""
    s = np.asarray(s)
    w = spectrogram_weights(frame_length)
    v = s.astype(np.float64)
    total = np.zeros(s.shape[:-2] + (s.shape[-1],), np.float64)
    for k in range(s.shape[-2]):
        total = total + np.square(v[..., k, :]) * w[k]
    power = (total * 2.0) / (float(frame_length) * float(frame_length))
    return np.sqrt(power)[..., None, :].astype(s.dtype)


# ---- inputs ------------------------------------------------------------------------------------------------------------------

def golden_signal(params):
    """energy_goldens.ml:31-38"""
    channels, length = params["channels"], params["length"]
    v = lcg_values(channels * length).astype(params["dtype"])
    return v.reshape(channels, length) if channels > 1 else v


def golden_spectrogram(params):
    """energy_goldens.ml:40-50"""
    channels, bins, count = params["channels"], params["bins"], params["frames"]
    v = np.abs(lcg_values(channels * bins * count)).astype(params["dtype"])
    return v.reshape(channels, bins, count) if channels > 1 else v.reshape(bins, count)


def decades(seed, clips, n, dtype):
    """noise scaled over 12 decades: the order of a float64 sum of its squares matters"""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((clips, n)) * 10.0 ** rng.uniform(-6.0, 6.0, size=(clips, n))).astype(dtype)
