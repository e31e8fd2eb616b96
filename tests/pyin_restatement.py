"""numpy restatement of pYIN (include/soundml_amd.h words the definition), no GPU.  It builds on pitch_restatement:
yin's d' with its chains and its bits.  Every add and every product is explicit and rounds on its own; the host tables (thr, beta,
E, Z, freq, edge, tri, rs: ``Pitch.pyin_tables``) are inputs.  This file is the yardstick of tests/test_gpu_pyin.py.

  observation   the troughs of d' (yin's rule without the threshold), p_r over the thresholds in ascending k with the ONE product
                Z[N] * E[q] rounded before it meets beta, the no-trough share on the first least trough (none where no threshold lies
                above it), the bins by counting edges,
                obs[b] in ascending r, voiced_prob in ascending b
  decode        probability domain: B = max(obs, 2^-200), a rescale by a power of two per frame, candidates u[i] * tri[j - i + h] in
                ascending i with strict >, stay against switch with strict >, the smallest state of the greatest final delta"""
import numpy as np

import pitch_restatement as P

FLOOR = 2.0 ** -200
frames = P.frames


def troughs(dn, pmin, pmax):
    """one frame's d' -> [(tau, height, shift)] in ascending tau"""
    out = []
    for tau in range(pmin, pmax + 1):
        if dn[tau] <= dn[tau - 1] and (tau == pmax or dn[tau] < dn[tau + 1]):
            shift = 0.0
            if tau - 1 >= 1 and tau + 1 <= pmax:
                a, b, c = dn[tau - 1], dn[tau], dn[tau + 1]
                den = (a - 2.0 * b) + c
                if den > 0.0:
                    s = (0.5 * (a - c)) / den
                    if abs(s) <= 1.0:
                        shift = s
            out.append((tau, dn[tau], shift))
    return out


def frame_observation(dn, pmin, pmax, sample_rate, tab, no_trough_prob):
    """one frame's d' -> (obs [2 n_bins], voiced_prob)"""
    thr, beta, E, Z, edge = tab["thr"], tab["beta"], tab["E"], tab["Z"], tab["edge"]
    n, n_bins = beta.size, tab["freq"].size
    found = troughs(dn, pmin, pmax)
    g = np.array([t[1] for t in found], np.float64)
    p = np.zeros(len(found), np.float64)
    for k in range(1, n + 1):
        below = g < thr[k]
        N = int(below.sum())
        if N == 0:
            continue
        q = np.cumsum(below) - below                       # the troughs below before this one
        add = (Z[N] * E[q]) * beta[k - 1]
        p = np.where(below, p + add, p)
    if len(found):
        star = int(np.argmin(g))                           # the first of the least
        K0 = int((thr[1:] <= g[star]).sum())
        if K0 < n:                                         # a threshold lies above the least trough (not so where d' = 1: silence)
            share = 0.0
            for k in range(K0):
                share = share + beta[k]
            p[star] = p[star] + no_trough_prob * share
    obs = np.zeros(2 * n_bins, np.float64)
    for r, (tau, _, shift) in enumerate(found):
        if p[r] > 0.0:
            f = float(sample_rate) / (float(tau) + shift)
            b = int(np.searchsorted(edge, f, side="right"))    # the number of edges <= f
            obs[b] = obs[b] + p[r]
    vp = 0.0
    for b in range(n_bins):
        vp = vp + obs[b]
    vp = min(1.0, vp)
    obs[n_bins:] = (1.0 - vp) / float(n_bins)
    return obs, vp


def observation(x, fmin, fmax, sample_rate, frame_length, hop, tab, no_trough_prob=0.01):
    """[...; n] -> float64 (obs [...; count; 2 n_bins] as the decoder sees it, voiced_prob [...; count], sound [...; count])"""
    pmin, pmax = P.lag_range(sample_rate, fmin, fmax, frame_length)
    dn, e0, c = P.normalised(P.padded_frames(x, frame_length, hop), hop, pmax)
    flat = dn.reshape(-1, pmax + 1)
    sound = (np.isfinite(e0) & np.isfinite(c)).reshape(-1)
    n_bins = tab["freq"].size
    obs, vp = np.zeros((flat.shape[0], 2 * n_bins), np.float64), np.zeros(flat.shape[0], np.float64)
    for i in range(flat.shape[0]):
        if sound[i]:
            obs[i], vp[i] = frame_observation(flat[i], pmin, pmax, sample_rate, tab, no_trough_prob)
        else:
            obs[i, n_bins:] = 1.0 / float(n_bins)              # a zero voiced part and voiced_prob = 0 for the decoder
    lead = dn.shape[:-1]
    return obs.reshape(lead + (2 * n_bins,)), vp.reshape(lead), sound.reshape(lead)


def decode(obs, tri, rs, switch_prob=0.01, return_delta=False):
    """one clip: float64 obs [2 n_bins; T] -> int states [T]"""
    S, T = obs.shape
    nb, h = S // 2, (tri.size - 1) // 2
    keep = 1.0 - switch_prob
    with np.errstate(invalid="ignore"):
        B = np.where(obs > FLOOR, obs, FLOOR)
    p_init = np.concatenate([np.zeros(nb), np.full(nb, 1.0 / float(nb))])
    delta = p_init * B[:, 0]
    back = np.zeros((T, S), np.int64)
    for t in range(1, T):
        _, e = np.frexp(delta.max())
        u = ((delta * np.ldexp(1.0, -int(e))) * np.concatenate([rs, rs])).reshape(2, nb)
        best = np.full((2, nb), -np.inf)
        arg = np.tile(np.arange(nb), (2, 1))
        for k in range(min(2 * h, h + nb - 1), max(-1, h - nb), -1):      # ascending i = j - k + h
            j0, j1 = max(0, k - h), min(nb, nb + k - h)
            cand = u[:, j0 - k + h:j1 - k + h] * tri[k]
            take = cand > best[:, j0:j1]
            best[:, j0:j1] = np.where(take, cand, best[:, j0:j1])
            arg[:, j0:j1] = np.where(take, np.arange(j0 - k + h, j1 - k + h)[None, :], arg[:, j0:j1])
        new = np.empty(S)
        for v in (0, 1):
            stay, change = best[v] * keep, best[1 - v] * switch_prob
            sw = change > stay
            new[v * nb:(v + 1) * nb] = np.where(sw, change, stay) * B[v * nb:(v + 1) * nb, t]
            back[t, v * nb:(v + 1) * nb] = np.where(sw, (1 - v) * nb + arg[1 - v], v * nb + arg[v])
        delta = new
    states = np.zeros(T, np.int64)
    states[T - 1] = int(np.argmax(delta))                      # the first of the greatest
    for t in range(T - 1, 0, -1):
        states[t - 1] = back[t, states[t]]
    return (states, delta) if return_delta else states


def pyin_decode(obs, tri, rs, switch_prob=0.01):
    """[...; 2 n_bins; T] -> states [...; 1; T] in the dtype of obs"""
    obs = np.asarray(obs)
    flat = obs.reshape((-1,) + obs.shape[-2:]).astype(np.float64)
    out = np.stack([decode(c, tri, rs, switch_prob) for c in flat]) if flat.shape[0] else np.zeros((0, obs.shape[-1]))
    return out.reshape(obs.shape[:-2] + (1, obs.shape[-1])).astype(obs.dtype)


def pyin_observation(x, fmin, fmax, tab, sample_rate=22050, frame_length=2048, hop=None, no_trough_prob=0.01):
    """[...; n] -> [...; 2 n_bins; count] in the dtype of x, NaN columns where a frame holds a non-finite sample"""
    hop = frame_length // 4 if hop is None else hop
    obs, _, sound = observation(x, fmin, fmax, sample_rate, frame_length, hop, tab, no_trough_prob)
    obs = np.where(sound[..., None], obs, np.nan)
    return np.ascontiguousarray(np.swapaxes(obs, -1, -2)).astype(np.asarray(x).dtype)


def pyin(x, fmin, fmax, tab, sample_rate=22050, frame_length=2048, hop=None, switch_prob=0.01, no_trough_prob=0.01, fill_na=np.nan,
         return_states=False):
    """[...; n] -> (f0, voiced_flag, voiced_prob), each [...; 1; count] in the dtype of x"""
    hop = frame_length // 4 if hop is None else hop
    dtype = np.asarray(x).dtype
    obs, vp, sound = observation(x, fmin, fmax, sample_rate, frame_length, hop, tab, no_trough_prob)
    lead, count, nb = obs.shape[:-2], obs.shape[-2], tab["freq"].size
    flat = obs.reshape((-1, count, 2 * nb))
    states = np.stack([decode(c.T, tab["tri"], tab["rs"], switch_prob) for c in flat]).reshape(lead + (1, count))
    voiced = states < nb
    f0 = tab["freq"][states % nb]
    if fill_na is not None:
        f0 = np.where(voiced, f0, fill_na)
    prob = np.where(sound, vp, np.nan).reshape(lead + (1, count))
    out = f0.astype(dtype), voiced.astype(dtype), prob.astype(dtype)
    return out + (states,) if return_states else out


# ---- crafted observations of the decoder's edge cases: (obs [2 n_bins; T], h) -----------------------------------------------------

def _with_rest(obs, nb):
    obs[nb:] = (1.0 - obs[:nb].sum(axis=0)) / float(nb)
    return obs


def crafted_equal_candidates(nb=21, h=3, T=6):
    """two equal candidates in every frame, both interior (the same rs): every voiced path through bin 8 ties with one through 10"""
    obs = np.zeros((2 * nb, T))
    obs[8] = obs[10] = 0.375
    return _with_rest(obs, nb), h


def crafted_jump(nb=21, h=3):
    """voiced_prob = 1 in every frame; the one candidate jumps from bin 2 to bin 15, further than the band"""
    obs = np.zeros((2 * nb, 6))
    obs[2, :2] = 1.0
    obs[15, 2:] = 1.0
    return _with_rest(obs, nb), h


def crafted_short(T, nb=9, h=2):
    rng = np.random.default_rng(T)
    obs = np.zeros((2 * nb, T))
    obs[:nb] = rng.uniform(0.0, 0.9 / nb, (nb, T))
    obs[nb:] = rng.uniform(0.0, 0.1, (nb, T))              # not uniform over the unvoiced states: the end state is a choice
    return obs, h


def crafted_wide(nb, h=4, T=5):
    """more bins than a workgroup has lanes: a lane owns a run of them"""
    rng = np.random.default_rng(nb)
    obs = np.zeros((2 * nb, T))
    obs[:nb] = rng.uniform(0.0, 0.5, (nb, T)) * (rng.uniform(0.0, 1.0, (nb, T)) < 0.02)
    obs[nb:] = rng.uniform(0.0, 1e-3, (nb, T))
    return obs, h
