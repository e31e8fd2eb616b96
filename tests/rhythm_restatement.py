"""numpy restatement of Rhythm (include/soundml_amd.h words the definitions, DESIGN.md 4.8g the orders), no GPU.  Every add is
explicit: nothing is left to numpy's pairwise sums, and numpy never fuses a product with a sum.  The transcendental tables (the
window, the prior, g and tx) are INPUTS: the tests pass the library's own, so that the device is compared bit for bit and nothing
hangs on libm's last ulp; test_rhythm_restatement.py pins the tables to the numpy formulas."""
import numpy as np

DBL_MIN = np.finfo(np.float64).tiny

# (frames, p, win_length, sample_rate, hop): the click tracks; an odd window; frames < window; the default window
GEOMETRIES = [(96, 8, 32, 8000, 500), (200, 20, 64, 22050, 512), (61, 5, 16, 8000, 800), (40, 8, 33, 8000, 500), (7, 3, 8, 8000, 1000),
              (431, 21, 384, 22050, 512)]


def clicks(frames, p):
    return np.arange(3, frames, p)


def click_batch(geometry, dtype=np.float32):
    """[3; frames]: the click track (0.05 x uniform noise, 1.0 added at frames 3, 3 + p, ..), then two clips of noise scaled by 1e-6
    and by 1e6"""
    frames, p = geometry[:2]
    rng = np.random.default_rng(1000 * frames + p)
    x = rng.random((3, frames))
    x[0] *= 0.05
    x[0, clicks(frames, p)] += 1.0
    x[1] *= 1e-6
    x[2] *= 1e6
    return x.astype(np.float32).astype(dtype)


def half_even(p):
    """round_half_even(p / 2) of an integer p"""
    k = p // 2
    return k + (k & 1) if p & 1 else k


# ---- tempogram ----------------------------------------------------------------------------------------------------------------

def frames_of(env, w):
    """y [lead; frames; W] in float64: y_j = w_j pad[t + j], the envelope extended by W // 2 zeros on the left and W - W // 2 on the right"""
    env = np.asarray(env)
    W, frames = len(w), env.shape[-1]
    pad = np.zeros(env.shape[:-1] + (frames + W,), np.float64)
    pad[..., W // 2:W // 2 + frames] = env
    index = np.arange(frames)[:, None] + np.arange(W)[None, :]
    return np.asarray(w, np.float64) * pad[..., index]


def autocorrelation(y, descending=False):
    """a [..; W]: a(tau) = sum_{j < W - tau} y_j y_{j + tau}, one chain over j from 0.0, ascending (descending: the other order, which
    test_rhythm_restatement.py shows to give other bits)"""
    W = y.shape[-1]
    a = np.zeros(y.shape, np.float64)
    for j in (range(W - 1, -1, -1) if descending else range(W)):
        a[..., :W - j] = a[..., :W - j] + y[..., j:j + 1] * y[..., j:]
    return a


def tempogram_wide(env, w, norm=True):
    """[lead; frames; W] in float64, before the rounding"""
    with np.errstate(all="ignore"):
        a = autocorrelation(frames_of(env, w))
        if norm:
            a0 = a[..., :1]
            a = np.where(a0 < DBL_MIN, a, a / a0)                # a NaN a(0) divides too
    return a


def tempogram(env, w, norm=True):
    """[lead; W; frames] in the dtype of env"""
    env = np.asarray(env)
    with np.errstate(all="ignore"):
        return np.ascontiguousarray(np.swapaxes(tempogram_wide(env, w, norm), -1, -2).astype(env.dtype))


# ---- tempo --------------------------------------------------------------------------------------------------------------------

def tempo_scores(wide, prior):
    """(m, score) [lead; W] of the float64 normalised tempogram [lead; frames; W]: the frame mean as one ascending chain, one division"""
    frames = wide.shape[-2]
    m = np.zeros(wide.shape[:-2] + wide.shape[-1:], np.float64)
    with np.errstate(all="ignore"):
        for t in range(frames):
            m = m + wide[..., t, :]
        m = m / np.float64(frames)
        return m, np.log1p(1e6 * m) + prior


def pick(score, prior):
    """(lag, gap): the smallest admissible lag that attains the greatest score that is a number (0: none), and how far the
    best other score lies below it"""
    lag, best = 0, None
    for tau in range(len(score)):
        if prior[tau] > -np.inf and score[tau] == score[tau] and (lag == 0 or score[tau] > best):
            lag, best = tau, score[tau]
    others = [score[tau] for tau in range(len(score)) if tau != lag and prior[tau] > -np.inf and score[tau] == score[tau]]
    return lag, (best - max(others)) if lag and others else np.inf


def tempo_lag(env, w, prior):
    """(lags [lead], gaps [lead]); lag 0 where the clip has none (m(1) is NaN, or no score is a number)"""
    env = np.asarray(env)
    m, score = tempo_scores(tempogram_wide(env, w, True), prior)
    lags, gaps = [], []
    for c in range(env.shape[0]):
        lag, gap = pick(score[c], prior)
        if len(prior) < 2 or m[c, 1] != m[c, 1]:
            lag, gap = 0, np.inf
        lags.append(lag)
        gaps.append(gap)
    return np.array(lags), np.array(gaps)


# ---- the beat tracker ---------------------------------------------------------------------------------------------------------

def deviation(env):
    """sd with ddof = 1: the mean and the squared deviations as ascending chains"""
    n = len(env)
    s = np.float64(0.0)
    for v in env:
        s = s + v
    mean = s / np.float64(n)
    q = np.float64(0.0)
    for v in env:
        d = v - mean
        q = q + d * d
    return np.sqrt(q / np.float64(n - 1))


def local_score(ne, g, period):
    """ls_i = sum_n ne_n g(i - n), n ascending over the clip's own indices within `period` of i"""
    frames = len(ne)
    ls, at = np.zeros(frames, np.float64), np.arange(frames)
    for s in range(2 * period + 1):
        n = at - period + s
        ok = (n >= 0) & (n < frames)
        ls[ok] = ls[ok] + ne[n[ok]] * g[2 * period - s]
    return ls


def recursion(ls, tx, period):
    """(cum, back)"""
    frames = len(ls)
    window = -2 * period + np.arange(len(tx))
    cum, back = np.zeros(frames, np.float64), np.full(frames, -1, np.int64)
    enough, started = 0.01 * ls.max(), False
    for i in range(frames):
        at = i + window
        cand = np.where(at >= 0, tx + cum[np.clip(at, 0, frames - 1)], tx)
        k = int(np.argmax(cand))                                 # the first of equals
        cum[i] = ls[i] + cand[k]
        started = started or ls[i] >= enough
        back[i] = i + window[k] if started else -1
    return cum, back


def maxima_of(cum):
    frames = len(cum)
    return [i for i in range(1, frames) if cum[i] > cum[i - 1] and (i == frames - 1 or cum[i] >= cum[i + 1])]


def median(values):
    """exact selection; the two middle values averaged for an even count"""
    v = np.sort(np.asarray(values, np.float64))
    n = len(v)
    return v[n // 2] if n & 1 else (v[n // 2 - 1] + v[n // 2]) / np.float64(2.0)


def beats_of(env, period, g, tx, trim=True):
    """the beat frames of ONE clip, ascending"""
    env = np.asarray(env, np.float64)
    frames = len(env)
    none = np.zeros(0, np.int64)
    if frames < 2 or period < 1:
        return none
    with np.errstate(all="ignore"):
        sd = deviation(env)
        if not (sd > 0.0 and sd < np.inf):
            return none
        ls = local_score(env / sd, g, period)
        if not np.all(np.isfinite(ls)):
            return none
        cum, back = recursion(ls, tx, period)
    peaks = maxima_of(cum)
    if not peaks:
        return none
    med = median(cum[peaks])
    last = [i for i in peaks if 2.0 * cum[i] > med]
    if not last:
        return none
    beats, i = [], last[-1]
    while i >= 0:
        beats.append(i)
        i = back[i]
    beats = np.array(beats[::-1], np.int64)
    v, nb = ls[beats], len(beats)
    sm = np.zeros(nb, np.float64)
    for q in range(nb):
        s = 0.5 * v[q - 1] + v[q] if q > 0 else v[q]
        sm[q] = s + 0.5 * v[q + 1] if q < nb - 1 else s
    th = np.float64(0.0)
    if trim:
        ss = np.float64(0.0)
        for s in sm:
            ss = ss + s * s
        th = 0.5 * np.sqrt(ss / np.float64(nb))
    keep = np.flatnonzero(sm > th)
    return beats[keep[0]:keep[-1] + 1] if len(keep) else none


def mask_of(beats, frames, dtype):
    out = np.zeros(frames, dtype)
    out[beats] = 1
    return out
