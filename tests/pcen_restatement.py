"""numpy restatement of Pcen (include/soundml_amd.h words the definition, DESIGN.md 4.8m the order), no GPU.  Every product, quotient
and sum is a float64 operation of its own, the rows are vectorised and time is a Python loop: the plain recurrence, nothing cut into
blocks.  The elementary functions are numpy's (the platform's libm), which hold a few float64 ulps as the device library's do."""
import numpy as np

DEFAULTS = dict(sr=22050, hop=512, gain=0.98, bias=2.0, power=0.5, time_constant=0.4, eps=1e-6, b=None, scale=1.0)


def params(**kw):
    p = dict(DEFAULTS)
    p.update(kw)
    return p


def coefficient(sr=22050, hop=512, time_constant=0.4, b=None, **_):
    if b is not None:
        return np.float64(b)
    T = np.float64(time_constant) * np.float64(sr) / np.float64(hop)
    TT = T * T
    return (np.sqrt(np.float64(1.0) + np.float64(4.0) * TT) - np.float64(1.0)) / (np.float64(2.0) * TT)


def smooth(S, s, scale=1.0, zi=None):
    """-> (u, M, zf): u = scale * S and M[t] = a M[t-1] + s u[t] in float64, [...; frames]; M[-1] = zi, or u[0]"""
    s = np.float64(s)
    a = np.float64(1.0) - s
    u = np.float64(scale) * np.asarray(S).astype(np.float64)
    M = np.empty_like(u)
    prev = u[..., 0].copy() if zi is None else np.array(zi, dtype=np.float64)
    for t in range(u.shape[-1]):
        keep = a * prev
        take = s * u[..., t]
        prev = keep + take
        M[..., t] = prev
    return u, M, prev


def compress(u, M, gain, bias, power, eps):
    """librosa's stable form, the operations in the stated order"""
    gain, bias, power, eps = (np.float64(v) for v in (gain, bias, power, eps))
    log_eps = np.log(eps)
    with np.errstate(divide="ignore", invalid="ignore"):
        sm = np.exp(-gain * (log_eps + np.log1p(M / eps)))
        if power == 0:
            return np.log1p(u * sm / bias)
        if bias == 0:
            return np.where(u == 0, np.float64(0.0), np.exp(power * (np.log(u) + np.log(sm))))
        return (bias ** power) * np.expm1(power * np.log1p(u * sm / bias))


def pcen(S, zi=None, **kw):
    """-> (P, M, zf), all float64 [...; frames] / [...]: round P (or M) once to the dtype of S to compare with the device"""
    p = params(**kw)
    u, M, zf = smooth(S, coefficient(**p), p["scale"], zi)
    return compress(u, M, p["gain"], p["bias"], p["power"], p["eps"]), M, zf


def inputs(seed, lead, bands, frames):
    """a non-negative float32 spectrogram [lead; bands; frames] over many decades: rng.random ** 8 times a per-row factor from 1e-6
    to 1e3, one all-zero row, a run of leading zeros in another, 2 % of the cells zero"""
    rng = np.random.default_rng(seed)
    S = rng.random((lead, bands, frames)) ** 8
    S *= 10.0 ** rng.uniform(-6.0, 3.0, size=(lead, bands, 1))
    S[rng.random(S.shape) < 0.02] = 0.0
    S[lead - 1, bands - 1, :] = 0.0
    S[0, 0, :max(1, frames // 4)] = 0.0
    return np.ascontiguousarray(S.astype(np.float32))


# the parameter sets of the device tests: each runs at scale 1 and 2**31
SETS = {
    "defaults": dict(),
    "gain.8-bias10-power.25": dict(gain=0.8, bias=10.0, power=0.25),
    "power0": dict(power=0.0),
    "bias0": dict(bias=0.0),
    "gain.5-bias1-power1-eps1e-3": dict(gain=0.5, bias=1.0, power=1.0, eps=1e-3),
}
SCALES = [1.0, 2.0 ** 31]
# (lead, bands, frames): rows that are no multiple of 64, partial last tiles, one row and one frame
SHAPES = [(3, 43, 321), (1, 1, 1), (2, 5, 63), (2, 5, 64), (1, 130, 65), (1, 64, 129), (5, 128, 431)]
