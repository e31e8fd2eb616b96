"""The numpy restatement of Decompose (tests/decompose_restatement.py) against what multiplicative updates must do, the host side
of the module (initial factors, argument errors worded by the ABI, checked with null pointers: no GPU), and the ctypes table
against the header."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import soundml_amd as S
from soundml_amd import Decompose, _lib
from conftest import GOLDEN, ROOT

import decompose_restatement as R

BETAS = (R.FROBENIUS, R.KL)
SMALL = [(33, 37, 3), (129, 70, 5), (40, 1, 1)]


def objective(V, W, H, beta):
    return R.divergence(V.astype(np.float64), W.astype(np.float64), H.astype(np.float64), beta)[..., 0]


def test_the_stated_order_is_the_accumulator_tile_order():
    """position 2 r + h of a 32-block is row (r & 3) + 8 (r >> 2) + 4 h: register r, lane half h of a 32 x 32 accumulator tile"""
    assert [R.perm32(i) for i in range(16)] == [0, 4, 1, 5, 2, 6, 3, 7, 8, 12, 9, 13, 10, 14, 11, 15]
    assert sorted(R.perm32(i) for i in range(32)) == list(range(32))
    steps = R.order32(70)
    assert len(steps) == 96 and sorted(s for s in steps if s >= 0) == list(range(70)) and steps.count(-1) == 26
    assert steps[64:72] == [64, 68, 65, 69, 66, -1, 67, -1]
    assert R.order_k(4) == [0, 1, 2, 3] and R.order_k(3) == [0, 1, 2, -1]


def test_float32_chain_is_the_stated_order_and_no_other():
    """the float32 restatement rounds after every term: it is within float32 rounding of the float64 one, and the ascending order
    gives other bits on the same data"""
    rng = np.random.default_rng(3)
    W, V = rng.random((2, 70, 5)).astype(np.float32), rng.random((2, 70, 9)).astype(np.float32)
    got, wide = R.inner_f(W, V, np.float32), R.inner_f(W, V, np.float64)
    assert got.dtype == np.float32 and np.abs(got - wide).max() <= 70 * 2.0 ** -24 * wide.max()
    asc = np.zeros(got.shape, np.float32)
    for f in range(70):
        asc = (W[:, f, :, None].astype(np.float64) * V[:, f, None, :] + asc).astype(np.float32)
    assert np.abs(asc - wide).max() <= 70 * 2.0 ** -24 * wide.max() and (asc != got).any()
    # one explicit scalar chain
    acc = np.float32(0)
    for f in R.order32(70):
        acc = np.float32(np.float64(W[1, f, 2]) * np.float64(V[1, f, 4]) + np.float64(acc)) if f >= 0 else acc
    assert acc == got[1, 2, 4]


@pytest.mark.parametrize("beta", BETAS)
@pytest.mark.parametrize("geometry", SMALL)
def test_objective_never_rises_in_float64(geometry, beta):
    V = R.problem(geometry, clips=2)
    snaps = R.nmf(V, *R.initial((2,), *geometry), 200, beta, np.float64, (0, 1, 2, 8, 50, 200))
    obj = [objective(V, *snaps[r], beta) for r in (0, 1, 2, 8, 50, 200)]
    print(geometry, beta, [o.tolist() for o in obj])
    for before, after in zip(obj, obj[1:]):
        assert np.all(after <= before * (1 + 1e-12) + 1e-15), (before, after)
    for W, H in snaps.values():
        assert W.min() >= 0 and H.min() >= 0


@pytest.mark.parametrize("beta", BETAS)
def test_an_exact_product_is_recovered(beta):
    """V = W* H* exactly with K = K*: the relative Frobenius objective falls far below where it starts"""
    rng = np.random.default_rng(5)
    Wt, Ht = rng.random((2, 48, 4)) ** 2, rng.random((2, 4, 40)) ** 2
    V = Wt @ Ht
    W0, H0 = R.initial((2,), 48, 40, 4)
    W, H = R.nmf(V, W0, H0, 2000, beta, np.float64)
    start, end = objective(V, W0, H0, R.FROBENIUS), objective(V, W, H, R.FROBENIUS)
    print(beta, "relative Frobenius objective", start.tolist(), "->", end.tolist(), "factor", (start / end).tolist())
    assert np.all(end < start / 50)


def test_float32_restatement_stays_near_float64():
    g = (65, 64, 32)
    V = R.problem(g, clips=2)
    W0, H0 = R.initial((2,), *g)
    for beta in BETAS:
        a, b = R.nmf(V, W0, H0, 8, beta, np.float64), R.nmf(V, W0, H0, 8, beta, np.float32)
        for x, y in zip(a, b):
            assert y.dtype == np.float32 and np.abs(x - y).max() / x.max() < 1e-5


def test_reconstruct_and_divergence_restated():
    rng = np.random.default_rng(9)
    W, H = rng.random((3, 10, 5)), rng.random((3, 5, 7))
    assert np.allclose(R.reconstruct(W, H), W @ H, rtol=1e-14)
    assert np.array_equal(R.reconstruct(W, H, range(5)), R.reconstruct(W, H))
    assert np.allclose(R.reconstruct(W, H, [3, 1]), W[..., [1, 3]] @ H[..., [1, 3], :], rtol=1e-14)
    m = R.reconstruct(W, H, [0], as_mask=True) + R.reconstruct(W, H, [1, 2, 3, 4], as_mask=True)
    assert np.allclose(m, 1.0, rtol=1e-14)
    V = W @ H + 0.1 * rng.random((3, 10, 7))
    X = W @ H
    assert np.allclose(R.divergence(V, W, H, R.FROBENIUS)[:, 0], np.sqrt(((V - X) ** 2).sum((1, 2)) / (V ** 2).sum((1, 2))), rtol=1e-13)
    kl = ((V * np.log(V / X)).sum((1, 2)) - V.sum((1, 2)) + X.sum((1, 2))) / V.sum((1, 2))
    assert np.allclose(R.divergence(V, W, H, R.KL)[:, 0], kl, rtol=1e-10, atol=1e-15)
    V[0, 0, 0] = 0.0                                                           # a zero of V adds nothing to the KL sum
    assert np.isfinite(R.divergence(V, W, H, R.KL)).all()


def test_golden_objectives_are_the_restatements():
    """tests/golden/decompose/objectives.json holds what the float64 restatement reaches (the GPU test's residual gate)"""
    with open(os.path.join(GOLDEN, "decompose", "objectives.json")) as fh:
        golden = json.load(fh)
    assert len(golden) == 7 * 2
    for g in SMALL[:2]:
        V = R.problem(g)
        for beta in BETAS:
            snaps = R.nmf(V, *R.initial((4,), *g), 200, beta, np.float64, R.SNAPSHOTS)
            for r in R.SNAPSHOTS:
                want = golden["%dx%dx%d/%s" % (g + (beta,))][str(r)]
                assert np.allclose(objective(V, *snaps[r], beta), want, rtol=1e-12, atol=1e-16), (g, beta, r)


def test_initial_factors():
    W0, H0 = Decompose.initial((2, 3), 7, 5, 4, seed=6)
    assert W0.shape == (2, 3, 7, 4) and H0.shape == (2, 3, 4, 5) and W0.dtype == np.float64
    assert W0.min() > 0 and W0.max() <= 1 and H0.min() > 0 and H0.max() <= 1
    w, h = R.initial((2, 3), 7, 5, 4, seed=6)
    assert np.array_equal(W0, w) and np.array_equal(H0, h)
    assert np.array_equal(W0, 1.0 - np.random.Generator(np.random.PCG64([6, 0])).random((2, 3, 7, 4)))
    # a leading slice of a batch starts from the batch's factors
    W1, H1 = Decompose.initial((1,), 7, 5, 4, seed=6)
    assert np.array_equal(W1[0], W0[0, 0]) and np.array_equal(H1[0], H0[0, 0])
    W4, H4 = Decompose.initial((4,), 7, 5, 4, seed=6)
    assert np.array_equal(W4, W0.reshape(6, 7, 4)[:4]) and np.array_equal(H4, H0.reshape(6, 4, 5)[:4])
    assert not np.array_equal(Decompose.initial((1,), 7, 5, 4, seed=7)[0], W1)


def test_argument_errors_carry_their_wording():
    """checked before any tensor is looked at: no device is needed"""
    V = np.ones((2, 6, 5), np.float32)
    cases = [
        (lambda: S.nmf(V, 0), "nmf: n_components is 0 (at least 1)"),
        (lambda: S.nmf(V, Decompose.MAX_K + 1), "nmf: n_components is 1025 (at most 1024)"),
        (lambda: S.nmf(V, 3, beta="itakura-saito"), "nmf: unknown beta 'itakura-saito' (one of frobenius, kullback-leibler)"),
        (lambda: S.nmf(V, 3, n_iter=-1), "nmf: n_iter is -1 (at least 0)"),
        (lambda: S.nmf(V.astype(np.float64), 3, n_iter=-2), "nmf: n_iter is -2 (at least 0)"),
        (lambda: S.nmf(np.ones(4, np.float32), 3), "nmf: V has rank 1 (a spectrogram is [...; F; T]: at least 2)"),
        (lambda: S.nmf(V, 3, W0=np.ones((3, 6, 3))), "nmf: W0 has shape [3, 6, 3] where V, K and the leading axes ask for [2, 6, 3]"),
        (lambda: S.nmf(V, 3, H0=np.ones((2, 3, 4))), "nmf: H0 has shape [2, 3, 4] where V, K and the leading axes ask for [2, 3, 5]"),
        (lambda: S.nmf_activations(V, np.ones((3, 6, 3), np.float32)),
         "nmf_activations: the leading axes of V are [2] and those of W are [3] (the clips must agree, or W is one [F; K])"),
        (lambda: S.nmf_activations(V, np.ones((6, 3), np.float32), n_iter=-1), "nmf_activations: n_iter is -1 (at least 0)"),
        (lambda: S.nmf_activations(V, np.ones((6, 3), np.float32), beta=2), "nmf_activations: unknown beta 2 (one of frobenius, kullback-leibler)"),
        (lambda: S.nmf_reconstruct(np.ones((2, 6, 3)), np.ones((2, 4, 5))), "nmf_reconstruct: W has 3 components and H has 4"),
        (lambda: S.nmf_reconstruct(np.ones((2, 6, 3)), np.ones((3, 3, 5))),
         "nmf_reconstruct: the leading axes of W are [2] and those of H are [3] (the clips must agree)"),
        (lambda: S.nmf_reconstruct(np.ones((2, 6, 3)), np.ones((2, 3, 5)), [0, 3]), "nmf_reconstruct: component 3 is outside [0, 3)"),
        (lambda: Decompose.mask(np.ones((2, 6, 3)), np.ones((2, 3, 5)), [-1]), "nmf_mask: component -1 is outside [0, 3)"),
        (lambda: S.nmf_divergence(V, np.ones((2, 6, 3)), np.ones((2, 3, 5)), beta="x"),
         "nmf_divergence: unknown beta 'x' (one of frobenius, kullback-leibler)"),
        (lambda: S.nmf_divergence(V, np.ones((2, 7, 3)), np.ones((2, 3, 5))), "nmf_divergence: V has shape [2, 6, 5] where the factors give [...; 7; 5]"),
    ]
    for call, message in cases:
        with pytest.raises(S.InvalidArgument) as e:
            call()
        assert str(e.value) == message
    # the ABI's own wording of what Python words first, and of the placement arguments
    lib, check = _lib.lib, _lib.check
    raw = [
        (lambda: lib.smx_nmf_f32(None, None, None, 0, 6, 5, 3, 1, 7, None, None), "nmf: unknown beta 7 (0: frobenius, 1: kullback-leibler)"),
        (lambda: lib.smx_nmf_f32(None, None, None, 0, 0, 5, 3, 1, 0, None, None), "nmf: V is 0 x 5 (at least 1 x 1)"),
        (lambda: lib.smx_nmf_f32(None, None, None, -1, 6, 5, 3, 1, 0, None, None), "nmf: -1 clips (at least 0)"),
        (lambda: lib.smx_nmf_vram_f32(None, 30, 4, None, 18, None, 15, 0, 6, 5, 3, 1, 0, None, 18, None, 15, None), "nmf: V's row pitch is 4 (at least 5)"),
        (lambda: lib.smx_nmf_vram_f32(None, 29, 5, None, 18, None, 15, 0, 6, 5, 3, 1, 0, None, 18, None, 15, None), "nmf: V's clip stride is 29 (at least 30)"),
        (lambda: lib.smx_nmf_vram_f32(None, 30, 5, None, 18, None, 15, 0, 6, 5, 3, 1, 0, None, 17, None, 15, None), "nmf: W's clip stride is 17 (at least 18)"),
        (lambda: lib.smx_nmf_activations_vram_f32(None, 30, 5, None, 0, None, 14, 0, 6, 5, 3, 1, 0, None, 15, None),
         "nmf_activations: H0's clip stride is 14 (at least 15)"),
        (lambda: lib.smx_nmf_reconstruct_vram_f32(None, 18, None, 15, 0, 6, 5, 3, None, 0, 0, None, 30, 4, None),
         "nmf_reconstruct: the output's row pitch is 4 (at least 5)"),
        (lambda: lib.smx_nmf_divergence_vram_f32(None, 30, 5, None, 18, None, 14, 0, 6, 5, 3, 0, None, None), "nmf_divergence: H's clip stride is 14 (at least 15)"),
    ]
    for call, message in raw:
        with pytest.raises(S.InvalidArgument) as e:
            check(call())
        assert str(e.value) == message


def test_empty_batches_and_exports():
    for dtype in (np.float32, np.float64):
        W, H = S.nmf(np.ones((0, 6, 5), dtype), 3)
        assert W.shape == (0, 6, 3) and H.shape == (0, 3, 5) and W.dtype == dtype and H.dtype == dtype
        assert S.nmf_activations(np.ones((0, 6, 5), dtype), np.ones((0, 6, 3), dtype)).shape == (0, 3, 5)
        assert S.nmf_reconstruct(np.ones((0, 6, 3), dtype), np.ones((0, 3, 5), dtype)).shape == (0, 6, 5)
        assert S.nmf_divergence(np.ones((0, 6, 5), dtype), np.ones((0, 6, 3), dtype), np.ones((0, 3, 5), dtype)).shape == (0, 1)
    assert S.Decompose.nmf is S.nmf and Decompose.TILE_K == 64 and Decompose.EPS == 2.0 ** -23
    for name in ("Decompose", "nmf", "nmf_activations", "nmf_reconstruct", "nmf_divergence"):
        assert name in S.__all__


def test_ctypes_signatures_agree_with_the_header():
    """every Decompose declaration: as many ctypes arguments as the header has parameters, in the header's order; the device forms
    end in _vram_f32, take a stride for every array and the stream last, and no older coverage law's pattern matches them"""
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "soundml_amd.h")).read(), flags=re.S)
    kinds = {"int64_t": C.c_int64, "double": C.c_double, "int": C.c_int}
    found = []
    for m in re.finditer(r"\bint (smx_nmf[a-z0-9_]*)\s*\(([^)]*)\)\s*;", header):
        name, params = m.group(1), [" ".join(p.split()) for p in m.group(2).split(",")]
        want = [C.c_void_p if "*" in p else kinds[p.split(" ")[0]] for p in params]
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int and args == want, name
        if "_vram" in name:
            assert name.endswith("_vram_f32") and params[-1] == "void *stream", name
            arrays = [p.split("*")[1] for p in params if p.startswith(("const float *d_", "float *d_"))]
            strides = [p.split(" ")[1] for p in params if p.endswith("_stride")]
            assert len(arrays) >= 3 and (len(strides) == len(arrays) or name == "smx_nmf_divergence_vram_f32"), (name, arrays, strides)
            assert not re.search(r"smx_\w+_dev\b|smx_\w+_device_f32\b|smx_\w+_dev_f(32|64)\b|smx_\w+_resident_f32\b|smx_\w+_gpu_f32\b|smx_\w+_hbm_f32\b",
                                 name), name
        found.append(name)
    assert len(found) == 13 and len([n for n in found if n.endswith("_vram_f32")]) == 4, found
    assert sorted(n for n in _lib.SIGNATURES if n.startswith("smx_nmf")) == sorted(found)
