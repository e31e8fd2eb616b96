"""nmf / nmf_activations / nmf_reconstruct / nmf_divergence on the device.

The yardsticks: the numpy restatement (tests/decompose_restatement.py) in float64 and in float32 in the stated order, the objectives
the float64 restatement reaches (tests/golden/decompose/objectives.json), and laws that hold bit for bit whatever the algorithm:
the two routes, slices, faces, continuation, the activations of a run, a shared dictionary, reconstruction.  Every figure a gate
compares is printed before the gate.

The geometries (F, T, K) are the smallest that break a tile kernel: one past a 32-block in both axes, K odd and over one 16-block,
whole blocks, one cell, the real row count at the tile cap, and one K above the cap (the general route).  A batch of 4 clips is drawn
once per geometry; leads (3,) and (2, 2) are its first three clips and all four, and so are their default initial factors."""
import functools
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import soundml_amd as S
from soundml_amd import Decompose
from conftest import GOLDEN, ROOT

import decompose_restatement as R

pytestmark = pytest.mark.gpu

TILE = [(33, 37, 3), (129, 70, 5), (257, 45, 17), (65, 64, 32), (40, 1, 1), (1025, 70, 64)]
GENERAL = (33, 37, Decompose.TILE_K + 1)
GEOMETRIES = TILE + [GENERAL]
LEADS = [(3,), (2, 2)]
ROUNDS = R.SNAPSHOTS
BETAS = (R.FROBENIUS, R.KL)


def dev(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()


def host(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)


def same_bits(got, want, what):
    got, want = host(got), host(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, got.dtype, want.shape, want.dtype)
    word = np.int32 if got.dtype == np.float32 else np.int64
    differ = np.ascontiguousarray(got).view(word) != np.ascontiguousarray(want).view(word)
    differ &= ~(np.isnan(got) & np.isnan(want))
    assert not differ.any(), "%s: %d/%d values differ, the first at %s: %r against %r" % (
        what, int(differ.sum()), differ.size, np.argwhere(differ)[0].tolist(), got[differ][0], want[differ][0])


@functools.lru_cache(maxsize=None)
def clips(geometry):
    V = R.problem(geometry)
    V.setflags(write=False)
    return V


def batch(geometry, lead):
    """V [lead; F; T] in float32: a leading slice of the geometry's four clips"""
    return clips(geometry)[:int(np.prod(lead))].reshape(lead + geometry[:2])


@functools.lru_cache(maxsize=None)
def restated(geometry, beta, dtype):
    """{round: (W, H)} of the four clips"""
    snaps = R.nmf(clips(geometry), *R.initial((4,), *geometry), max(ROUNDS), beta, np.dtype(dtype).type, ROUNDS)
    for pair in snaps.values():
        for a in pair:
            a.setflags(write=False)
    return snaps


def of_lead(a, lead):
    return a[:int(np.prod(lead))].reshape(lead + a.shape[1:])


@functools.lru_cache(maxsize=None)
def golden():
    with open(os.path.join(GOLDEN, "decompose", "objectives.json")) as fh:
        return json.load(fh)


def distance(got, want):
    return float(np.abs(got.astype(np.float64) - want).max() / want.max())


@pytest.mark.parametrize("beta", BETAS)
@pytest.mark.parametrize("lead", LEADS, ids=str)
@pytest.mark.parametrize("geometry", GEOMETRIES, ids=str)
def test_parity_with_the_restatement(geometry, lead, beta):
    """per factor max |got - want64| / max want64 stays within 4 x the distance of the stated-order float32 restatement from the
    float64 one (the factor of test_gpu_mel_invert.py); the objective never rises by more than the float32 restatement's does, and
    after 200 rounds it is at most 2.0 x the float64 restatement's + 1e-5"""
    V = batch(geometry, lead)
    Vd = dev(V)
    wide, narrow = restated(geometry, beta, "float64"), restated(geometry, beta, "float32")
    objective, narrow_objective = [], []
    for r in ROUNDS:
        W, H = S.nmf(Vd, geometry[2], n_iter=r, beta=beta)
        assert W.is_cuda and W.dtype == Vd.dtype and tuple(W.shape) == lead + (geometry[0], geometry[2]) and tuple(H.shape) == lead + (geometry[2], geometry[1])
        objective.append(host(S.nmf_divergence(Vd, W, H, beta)).astype(np.float64))
        narrow_objective.append(R.divergence(V.astype(np.float64), *[of_lead(a, lead).astype(np.float64) for a in narrow[r]], beta))
        for name, got, w64, w32 in zip("WH", (host(W), host(H)), wide[r], narrow[r]):
            w64, w32 = of_lead(w64, lead), of_lead(w32, lead)
            d, ref = distance(got, w64), distance(w32, w64)
            bits = int((got.view(np.int32) != w32.view(np.int32)).sum())
            print("%s %s %s round %d %s: distance %.3e, the float32 restatement's %.3e; %d/%d values differ in bits from it" % (
                geometry, lead, beta, r, name, d, ref, bits, got.size))
            assert got.min() >= 0, "a factor went negative"
            assert d <= 4 * ref, (name, r, d, ref)
            if r == 0:
                same_bits(got, w32, "n_iter = 0 returns the initial factors")
    rise = max([0.0] + [float((b - a).max()) for a, b in zip(narrow_objective, narrow_objective[1:])])
    print("objective per round %s: %s; the float32 restatement rises by at most %.3e" % (ROUNDS, [o.reshape(-1).tolist() for o in objective], rise))
    for a, b in zip(objective, objective[1:]):
        # the output is one float32: 2^-23 of the value; float32 factors resolve V no finer than 2^-23 of it
        assert np.all(b <= a + rise + 2.0 ** -22 * a + 2.0 ** -22), (a, b)
    want = np.array(golden()["%dx%dx%d/%s" % (geometry + (beta,))][str(max(ROUNDS))])[:int(np.prod(lead))].reshape(lead + (1,))
    print("objective after %d rounds %s against the float64 restatement's %s" % (max(ROUNDS), objective[-1].reshape(-1).tolist(), want.reshape(-1).tolist()))
    assert np.all(objective[-1] <= 2.0 * want + 1e-5)


@pytest.mark.parametrize("beta", BETAS)
@pytest.mark.parametrize("geometry", GEOMETRIES, ids=str)
def test_float64_host_face(geometry, beta):
    """within 1e-13 of the frame-wise maximum (of the clip's for W) of the float64 restatement"""
    lead = (2, 2) if geometry == TILE[0] else (3,)
    V = batch(geometry, lead).astype(np.float64)
    wide = restated(geometry, beta, "float64")
    for r in ROUNDS:
        W, H = S.nmf(V, geometry[2], n_iter=r, beta=beta)
        assert isinstance(W, np.ndarray) and W.dtype == np.float64 and H.dtype == np.float64
        wW, wH = of_lead(wide[r][0], lead), of_lead(wide[r][1], lead)
        dW = float((np.abs(W - wW) / wW.max((-2, -1), keepdims=True)).max())
        dH = float((np.abs(H - wH) / wH.max(-2, keepdims=True)).max())
        print("%s %s round %d: W %.3e H %.3e" % (geometry, beta, r, dW, dH))
        assert dW <= 1e-13 and dH <= 1e-13


CHILD = """
import sys
sys.path[:0] = [%r, %r]
import numpy as np
import soundml_amd as S
import test_gpu_decompose as T
out = {}
for g in T.TILE:
    V = T.dev(T.batch(g, (3,)))
    for beta in T.BETAS:
        for r in (2, 8):
            W, H = S.nmf(V, g[2], n_iter=r, beta=beta)
            out["%%dx%%dx%%d/%%s/%%d/W" %% (g + (beta, r))], out["%%dx%%dx%%d/%%s/%%d/H" %% (g + (beta, r))] = T.host(W), T.host(H)
        out["%%dx%%dx%%d/%%s/act" %% (g + (beta,))] = T.host(S.nmf_activations(V, W[0], n_iter=3, beta=beta))
np.savez(sys.argv[1], **out)
"""


def test_tile_route_equals_general_route():
    """SMX_DISABLE_FAST in a fresh process: a thread per cell from memory instead of the matrix instruction, the same bits"""
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "general.npz")
        subprocess.run([sys.executable, "-c", CHILD % (ROOT, os.path.join(ROOT, "tests")), path], check=True,
                       env=dict(os.environ, SMX_DISABLE_FAST="1"), timeout=300)
        general = dict(np.load(path))
    assert len(general) == len(TILE) * 2 * 5
    for g in TILE:
        V = dev(batch(g, (3,)))
        for beta in BETAS:
            for r in (2, 8):
                W, H = S.nmf(V, g[2], n_iter=r, beta=beta)
                same_bits(W, general["%dx%dx%d/%s/%d/W" % (g + (beta, r))], (g, beta, r, "W"))
                same_bits(H, general["%dx%dx%d/%s/%d/H" % (g + (beta, r))], (g, beta, r, "H"))
            same_bits(S.nmf_activations(V, W[0], n_iter=3, beta=beta), general["%dx%dx%d/%s/act" % (g + (beta,))], (g, beta, "activations"))


@pytest.mark.parametrize("beta", BETAS)
@pytest.mark.parametrize("geometry", [TILE[0], TILE[2], TILE[5], GENERAL], ids=str)
def test_laws_bit_for_bit(geometry, beta):
    F, T, K = geometry
    V = batch(geometry, (2, 2))
    Vd = dev(V)
    W8, H8 = S.nmf(Vd, K, n_iter=8, beta=beta)
    # a leading slice of the batch
    Ws, Hs = S.nmf(Vd[0], K, n_iter=8, beta=beta)
    same_bits(Ws, W8[0], "slice W")
    same_bits(Hs, H8[0], "slice H")
    W3, H3 = S.nmf(dev(batch(geometry, (3,))), K, n_iter=8, beta=beta)
    same_bits(W3, W8.reshape(4, F, K)[:3], "three clips W")
    same_bits(H3, H8.reshape(4, K, T)[:3], "three clips H")
    # the host float32 face
    Wh, Hh = S.nmf(V, K, n_iter=8, beta=beta)
    assert isinstance(Wh, np.ndarray) and Wh.dtype == np.float32
    same_bits(Wh, W8, "host face W")
    same_bits(Hh, H8, "host face H")
    # a run continued from its own factors
    W5, H5 = S.nmf(Vd, K, n_iter=5, beta=beta)
    W7, H7 = S.nmf(Vd, K, n_iter=2, beta=beta, W0=W5, H0=H5)
    Wc, Hc = S.nmf(Vd, K, n_iter=1, beta=beta, W0=W7, H0=H7)
    same_bits(Wc, W8, "continued W")
    same_bits(Hc, H8, "continued H")
    # the last H update of the run of 8 rounds is one round of nmf_activations from the run of 7
    same_bits(S.nmf_activations(Vd, W7, n_iter=1, beta=beta, H0=H7), H8, "activations")
    same_bits(S.nmf_activations(V, host(W7), n_iter=1, beta=beta, H0=host(H7)), H8, "activations, host face")
    # one dictionary for the batch against the same dictionary per clip
    D = W8[1, 0].contiguous()
    tiled = D.expand(2, 2, F, K).contiguous()
    shared = S.nmf_activations(Vd, D, n_iter=4, beta=beta)
    same_bits(shared, S.nmf_activations(Vd, tiled, n_iter=4, beta=beta), "shared dictionary")
    same_bits(S.nmf_activations(V, host(D), n_iter=4, beta=beta), shared, "shared dictionary, host face")
    # a view of a wider spectrogram is taken as it stands
    import torch
    wide = torch.full((2, 2, F, T + 5), float("nan"), device="cuda")
    wide[..., 2:T + 2] = Vd
    Wv, Hv = S.nmf(wide[..., 2:T + 2], K, n_iter=8, beta=beta)
    same_bits(Wv, W8, "view W")
    same_bits(Hv, H8, "view H")
    same_bits(S.nmf_divergence(wide[..., 2:T + 2], W8, H8, beta), S.nmf_divergence(Vd, W8, H8, beta), "view objective")


@pytest.mark.parametrize("geometry", [TILE[1], TILE[3], GENERAL], ids=str)
def test_reconstruct_and_mask(geometry):
    F, T, K = geometry
    Vd = dev(batch(geometry, (2, 2)))
    W, H = S.nmf(Vd, K, n_iter=8)
    X = S.nmf_reconstruct(W, H)
    assert tuple(X.shape) == (2, 2, F, T) and X.is_cuda
    same_bits(S.nmf_reconstruct(W, H, components=range(K)), X, "all components")
    same_bits(S.nmf_reconstruct(host(W), host(H)), X, "host face")
    w, h = host(W), host(H)
    want = R.reconstruct(w.astype(np.float64), h.astype(np.float64))
    bound = K * 2.0 ** -24 * want
    print("reconstruct: max error %.3e of the bound" % float((np.abs(host(X) - want) / bound).max()))
    assert np.all(np.abs(host(X) - want) <= bound)
    narrow = R.reconstruct(w, h)
    print("%d/%d values differ in bits from the float32 restatement" % (int((narrow.view(np.int32) != host(X).view(np.int32)).sum()), narrow.size))
    some = sorted({0, K // 2, K - 1})
    part = S.nmf_reconstruct(W, H, components=some[::-1])
    sub = R.reconstruct(w[..., some].astype(np.float64), h[..., some, :].astype(np.float64))
    assert np.all(np.abs(host(part) - sub) <= K * 2.0 ** -24 * np.maximum(sub, 2.0 ** -126))
    # the mask is that sum over floor(all), one IEEE division
    eps = np.float32(Decompose.EPS)
    full = host(X)
    same_bits(Decompose.mask(W, H, some), host(part) / np.where(full < eps, eps, full), "mask")
    rest = [k for k in range(K) if k not in some]
    if rest:
        total = host(Decompose.mask(W, H, some)).astype(np.float64) + host(Decompose.mask(W, H, rest))
        assert np.abs(total - 1).max() <= (K + 2) * 2.0 ** -23


@pytest.mark.parametrize("geometry", [TILE[0], TILE[2]], ids=str)
def test_divergence(geometry):
    """Frobenius bit for bit on float64 hosts; KL within 2^-50 of the sum of its terms' magnitudes (a few ulp of log per term)"""
    lead = (2, 2)
    V = batch(geometry, lead)
    for beta in BETAS:
        W, H = [of_lead(a, lead) for a in restated(geometry, beta, "float64")[8]]
        V64 = V.astype(np.float64)
        got = S.nmf_divergence(V64, W, H, beta)
        assert got.shape == lead + (1,) and got.dtype == np.float64
        want, scale = R.divergence(V64, W, H, beta, parts=True)
        print(geometry, beta, got.reshape(-1).tolist(), want.reshape(-1).tolist(), "difference", float(np.abs(got - want).max()))
        if beta == R.FROBENIUS:
            same_bits(got, want, "frobenius objective")
        else:
            assert np.all(np.abs(got - want) <= 2.0 ** -50 * scale)
        # float32 faces: the same float64 interior, one rounding
        w32, h32 = W.astype(np.float32), H.astype(np.float32)
        narrow = R.divergence(V, w32, h32, beta)
        got32 = S.nmf_divergence(V, w32, h32, beta)
        assert got32.dtype == np.float32
        assert np.all(np.abs(got32.astype(np.float64) - narrow) <= 2.0 ** -23 * np.abs(narrow))
        same_bits(S.nmf_divergence(dev(V), dev(w32), dev(h32), beta), got32, "device face")


@pytest.mark.parametrize("beta", BETAS)
@pytest.mark.parametrize("geometry", [TILE[1], TILE[5], GENERAL], ids=str)
def test_nan_stays_in_its_clip(geometry, beta):
    F, T, K = geometry
    V = np.array(batch(geometry, (3,)))
    clean = [S.nmf(dev(V), K, n_iter=r, beta=beta) for r in (2, 8)]
    V[1, F // 2, T // 2] = np.nan
    for (Wc, Hc), r in zip(clean, (2, 8)):
        W, H = S.nmf(dev(V), K, n_iter=r, beta=beta)
        assert np.isnan(host(W[1])).all() and np.isnan(host(H[1])).all()
        for c in (0, 2):
            same_bits(W[c], Wc[c], "the neighbour's W")
            same_bits(H[c], Hc[c], "the neighbour's H")


def test_refusals_on_the_device():
    import torch
    V = torch.ones((2, 6, 5), dtype=torch.float64, device="cuda")
    with pytest.raises(S.Failure) as e:
        S.nmf(V, 3)
    assert str(e.value) == "nmf: device-resident float64 spectrograms are not supported; pass a host array"
    with pytest.raises(S.InvalidArgument) as e:
        S.nmf(V.float(), 0)
    assert str(e.value) == "nmf: n_components is 0 (at least 1)"
    with pytest.raises(S.InvalidArgument) as e:
        S.nmf(V.float(), Decompose.MAX_K + 1)
    assert str(e.value) == "nmf: n_components is 1025 (at most 1024)"
    with pytest.raises(S.InvalidArgument) as e:
        S.nmf(V.float(), 3, W0=torch.ones((3, 6, 3), device="cuda"))
    assert str(e.value) == "nmf: W0 has shape [3, 6, 3] where V, K and the leading axes ask for [2, 6, 3]"
    with pytest.raises(S.InvalidArgument) as e:
        S.nmf(V.float(), 3, beta="is")
    assert str(e.value) == "nmf: unknown beta 'is' (one of frobenius, kullback-leibler)"
    with pytest.raises(S.InvalidArgument) as e:
        S.nmf(V.float(), 3, n_iter=-1)
    assert str(e.value) == "nmf: n_iter is -1 (at least 0)"
