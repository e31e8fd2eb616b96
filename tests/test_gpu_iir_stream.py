"""Iir.Kernel on the GPU: the concatenated steps and the flush equal Iir.apply of the whole signal BIT FOR BIT under every chunking,
on host chunks of both widths and on device chunks, on both routes; reset and reuse.  (Iir.apply itself is held against the
restatement by test_gpu_iir.py.)"""
import numpy as np
import pytest

from soundml_amd import Iir

import iir_restatement as R
from test_gpu_iir import B, W, device, route, same

pytestmark = pytest.mark.gpu

N = 2 * W * B + 3 * B + 5


def chunkings(n):
    yield "ones across a block edge", [B - 3] + [1] * 7 + [n - B - 4]
    yield "blocks", [B] * (n // B) + [n % B]
    yield "blocks and one", [B + 1] * (n // (B + 1)) + [n % (B + 1)]
    yield "spans", [W * B + 5, W * B, n - 2 * W * B - 5]
    yield "empties", [0, 5, 0, 0, n - 5, 0]
    rng = np.random.default_rng(5)
    cuts = sorted(set(rng.integers(0, n + 1, size=9).tolist()) | {0, n})
    yield "seeded", [b - a for a, b in zip(cuts[:-1], cuts[1:])]


def run(k, x, sizes):
    import torch
    parts, at = [], 0
    for m in sizes:
        out = k.step(x[..., at:at + m])
        assert (out is None) == (m == 0)
        if out is not None:
            assert tuple(out.shape) == tuple(x.shape[:-1]) + (m,)
            parts.append(out)
        at += m
    assert at == x.shape[-1] and k.position == at
    assert k.flush() == []
    return torch.cat(parts, dim=-1) if hasattr(parts[0], "is_cuda") else np.concatenate(parts, axis=-1)


@pytest.mark.parametrize("name", ["block", "general"])
@pytest.mark.parametrize("s", [1, 2, 4, 8])
def test_steps_equal_apply(s, name):
    c = Iir.Config.create(R.cascade(s))
    lead = (2, 3)
    x = R.batch(21, 6, N).reshape(lead + (N,))
    with route("block"):
        want = Iir.apply(c, x)
        want64 = Iir.apply(c, x.astype(np.float64))
    k = Iir.Kernel.prepare(c, *lead)
    with route(name):
        for what, sizes in chunkings(N):
            assert sum(sizes) == N
            if name == "general" and what not in ("ones across a block edge", "seeded"):
                continue
            k.reset()
            same(run(k, device(x), sizes), want, (s, name, what, "device chunks"))
            k.reset()
            same(run(k, x, sizes), want, (s, name, what, "host float32 chunks"))
            if what in ("seeded", "ones across a block edge"):
                k.reset()
                same(run(k, x.astype(np.float64), sizes), want64, (s, name, what, "host float64 chunks"))


def test_reset_and_reuse():
    import soundml_amd as S
    c = Iir.Config.create(R.cascade(2))
    x = device(R.batch(22, 3, 3 * B + 11))
    want = Iir.apply(c, x)
    k = Iir.Kernel.prepare(c, 3)
    first = run(k, x, [B + 7, 2 * B + 4])
    with pytest.raises(S.InvalidArgument, match="cannot feed a drained kernel"):
        k.step(x[..., :4])
    k.reset()
    assert k.position == 0
    k.step(x[..., :50])                     # an abandoned stream leaves nothing behind after reset
    k.reset()
    second = run(k, x, [5, 3 * B, 6])
    same(first, want.cpu().numpy(), "first use")
    same(second, want.cpu().numpy(), "after reset")
