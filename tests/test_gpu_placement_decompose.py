"""Placement of the Decompose device entry points: the rules of test_gpu_placement.py (guarded arena, an offset and row pads on V,
offsets on every factor and every output, row pads on the reconstruction, every output word written, no guard word touched, bit
equality with the ordinary call) for the entries whose names end in `_vram_f32`, which no older coverage law sees.  The gate is the
public call on packed tensors: a value taken from outside a row (the arena's NaN sentinel) reaches a factor within one update and
changes its bits.  Both routes run: the tile kernels read V's rows as 128-byte runs from wherever they start.  This file keeps a
table and a law of its own: every name of include/soundml_amd.h matching smx_\\w+_vram_f32 has a row here."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import soundml_amd as S
from soundml_amd import Decompose
from soundml_amd._lib import BETA, check, lib
from conftest import ROOT
from test_gpu_placement import Region, S_OUT, S_PAD, drive, environment, host, same      # noqa: F401  (the sentinels are the arena's)

import decompose_restatement as R

pytestmark = pytest.mark.gpu

TABLE = {}              # entry point -> the tests that place it
# (V offset, V row pad, first factor's offset, second factor's offset, output offset, output row pad) in elements
PLACEMENTS = [(0, 0, 0, 0, 0, 0), (1, 0, 2, 1, 1, 0), (3, 5, 1, 3, 3, 2), (2, 1, 3, 2, 0, 3), (0, 3, 0, 1, 2, 1)]
GEOMETRIES = [(33, 37, 3), (70, 45, 33)]         # one past a 32-block; two blocks of k
CLIPS = 3
ROUTES = [("tile", None), ("general", {"SMX_DISABLE_FAST": "1"})]
BETAS = (R.FROBENIUS, R.KL)


def row(*entries):
    def mark(fn):
        for e in entries:
            TABLE.setdefault(e, []).append(fn.__name__)
        return fn
    return mark


def call(name, *args, env=None):
    import torch
    assert name in TABLE, name
    raw = [a.ptr if isinstance(a, Region) else a for a in args]
    with environment(env):
        check(getattr(lib, name)(*raw, C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        torch.cuda.synchronize()
    for a in args:
        if isinstance(a, Region) and not a.output:
            a.intact()


def bit_gate(*wants):
    wants = [np.ascontiguousarray(w.cpu().numpy() if hasattr(w, "cpu") else w, np.float32).reshape(-1) for w in wants]

    def gate(res, pl):
        assert len(res) == len(wants)
        for k, want in enumerate(wants):
            got = host(res[k], np.float32).reshape(-1)
            differ = got.view(np.int32) != want.view(np.int32)
            assert not differ.any(), "%s: result %d: %d/%d values differ from the public call's, the first at %d" % (
                pl, k, int(differ.sum()), differ.size, int(np.argmax(differ)))
    return gate


def inputs(geometry):
    import torch
    V = R.problem(geometry, clips=CLIPS)
    W0, H0 = [a.astype(np.float32) for a in R.initial((CLIPS,), *geometry)]
    return V, W0, H0, torch.from_numpy(V).cuda()


@row("smx_nmf_vram_f32")
@pytest.mark.parametrize("route", ROUTES, ids=[r[0] for r in ROUTES])
@pytest.mark.parametrize("geometry", GEOMETRIES, ids=str)
def test_nmf(geometry, route):
    F, T, K = geometry
    V, W0, H0, Vd = inputs(geometry)
    for beta in BETAS:
        with environment(route[1]):
            want = S.nmf(Vd, K, n_iter=3, beta=beta)

        def run(pl):
            v, w0, h0 = Region.of(V, pl[0], pl[1]), Region.of(W0, pl[2]), Region.of(H0, pl[3])
            w, h = Region.out(1, CLIPS * F * K, np.float32, pl[4]), Region.out(1, CLIPS * K * T, np.float32, pl[2])
            call("smx_nmf_vram_f32", v, F * (T + pl[1]), T + pl[1], w0, F * K, h0, K * T, CLIPS, F, T, K, 3, BETA[beta], w, F * K, h, K * T, env=route[1])
            return [w.collect(), h.collect()]
        drive(run, PLACEMENTS, bit_gate(*want))


@row("smx_nmf_activations_vram_f32")
@pytest.mark.parametrize("route", ROUTES, ids=[r[0] for r in ROUTES])
@pytest.mark.parametrize("geometry", GEOMETRIES, ids=str)
def test_activations(geometry, route):
    F, T, K = geometry
    V, W0, H0, Vd = inputs(geometry)
    for beta in BETAS:
        for shared in (False, True):
            Wd = W0[1] if shared else W0
            with environment(route[1]):
                want = S.nmf_activations(Vd, Wd, n_iter=3, beta=beta)

            def run(pl):
                v, w, h0 = Region.of(V, pl[0], pl[1]), Region.of(Wd, pl[2]), Region.of(H0, pl[3])
                h = Region.out(1, CLIPS * K * T, np.float32, pl[4])
                call("smx_nmf_activations_vram_f32", v, F * (T + pl[1]), T + pl[1], w, 0 if shared else F * K, h0, K * T, CLIPS, F, T, K, 3, BETA[beta],
                     h, K * T, env=route[1])
                return [h.collect()]
            drive(run, PLACEMENTS, bit_gate(want))


@row("smx_nmf_reconstruct_vram_f32")
@pytest.mark.parametrize("geometry", GEOMETRIES, ids=str)
def test_reconstruct(geometry):
    F, T, K = geometry
    _, W0, H0, _ = inputs(geometry)
    some = (C.c_int64 * 2)(K - 1, 0)
    for comps, count, as_mask, want in ((None, 0, 0, S.nmf_reconstruct(W0, H0)), (some, 2, 0, S.nmf_reconstruct(W0, H0, [K - 1, 0])),
                                        (some, 2, 1, Decompose.mask(W0, H0, [0, K - 1]))):
        def run(pl):
            w, h = Region.of(W0, pl[2]), Region.of(H0, pl[3])
            out = Region.out(CLIPS * F, T, np.float32, pl[4], pl[5])
            call("smx_nmf_reconstruct_vram_f32", w, F * K, h, K * T, CLIPS, F, T, K, comps, count, as_mask, out, F * (T + pl[5]), T + pl[5])
            return [out.collect()]
        drive(run, PLACEMENTS, bit_gate(want))


@row("smx_nmf_divergence_vram_f32")
@pytest.mark.parametrize("geometry", GEOMETRIES, ids=str)
def test_divergence(geometry):
    F, T, K = geometry
    V, W0, H0, _ = inputs(geometry)
    for beta in BETAS:
        want = S.nmf_divergence(V, W0, H0, beta)

        def run(pl):
            v, w, h = Region.of(V, pl[0], pl[1]), Region.of(W0, pl[2]), Region.of(H0, pl[3])
            out = Region.out(1, CLIPS, np.float32, pl[4])
            call("smx_nmf_divergence_vram_f32", v, F * (T + pl[1]), T + pl[1], w, F * K, h, K * T, CLIPS, F, T, K, BETA[beta], out)
            return [out.collect()]
        drive(run, PLACEMENTS, bit_gate(want))


def test_coverage_law():
    """every device entry point of the header whose name ends in _vram_f32 runs in a row above (no GPU work)"""
    with open(os.path.join(ROOT, "include", "soundml_amd.h")) as fh:
        declared = set(re.findall(r"\b(smx_\w+_vram_f32)\s*\(", fh.read()))
    assert len(declared) >= 4
    missing = sorted(declared - set(TABLE))
    assert not missing, "device entry points without a placement row: %s" % ", ".join(missing)
    assert not sorted(set(TABLE) - declared)
