"""Resample.Config / Resample.apply / soundml_amd.resample and Resample.Kernel of a Config on the device.

1. DEFINITION: apply against the stage's float64 definition (oracle.resample_metrics.stage_polyphase on the float64
   prototype).  Tolerance per output, derived and not measured: (J + 2) 2^-24 sum_j |bank[p][j]| |x[q - j]|, J = 2 K + 1 --
   one rounding of each bank value to float32, at most J roundings along any summation order of exact fused products, one
   final rounding.  The sum is stage_polyphase on |proto| and |x|.  No output is excluded.
2. BIT EQUALITIES: batch = rows, host = device, strided = contiguous, Config = Stage on the overlap-save classes, the flat
   function = apply.
3. QUALITY: the float32 columns of the reference's decibel ruler (resample_quality.ml Q1-Q4), as
   tests/test_gpu_resample_quality.py asserts them for the pure classes.
4. STREAMING: the partition law, the emission count `ready` (resample.ml:1298), flush, reset, residence, errors."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import resample_metrics as M

import soundml_amd as S
from soundml_amd import Resample

EPS = 2.0 ** -24


def f32(x):
    return np.asarray(x, dtype=np.float64).astype(np.float32)


def check_definition(cfg, x, y):
    """every output of y = apply(cfg, x) within the derived bound of the float64 definition"""
    (l, m), k = cfg.rate, cfg.latency
    proto = cfg.prototype()
    y = np.asarray(y)
    assert y.dtype == np.float32 and y.shape == x.shape[:-1] + (-(-x.shape[-1] * l // m),)
    worst = 0.0
    for row, got in zip(x.reshape(-1, x.shape[-1]), y.reshape(-1, y.shape[-1])):
        want = M.stage_polyphase(proto, l, m, k, row)
        scale = M.stage_polyphase(np.abs(proto), l, m, k, np.abs(row))
        tol = (2 * k + 3) * EPS * scale
        err = np.abs(got.astype(np.float64) - want)
        bad = err > tol
        assert not bad.any(), "output %d: got %.9g, want %.9g, bound %.3g (%d of %d outside)" % (
            int(np.argmax(bad)), got[int(np.argmax(bad))], want[int(np.argmax(bad))], tol[int(np.argmax(bad))], int(bad.sum()), bad.size)
        worst = max(worst, float(np.max(err / np.maximum(tol, 1e-300))))
    return worst


# ---- 1. definition -------------------------------------------------------------------------------------------------------

RATIOS = [(44100, 48000), (48000, 44100), (44100, 16000), (3, 2), (5, 7)]


@pytest.mark.parametrize("sr,target", RATIOS)
def test_apply_is_the_stage_by_its_definition(sr, target):
    cfg = Resample.Config.create(sr, target)
    k = cfg.latency
    rng = np.random.default_rng(sr + target)
    for n in (1, k - 1, 2 * k + 1, 4999):
        x = rng.uniform(-1, 1, size=(3, n)).astype(np.float32)
        print(sr, target, n, "worst error / bound:", check_definition(cfg, x, Resample.apply(cfg, x)))


@pytest.mark.parametrize("sr,target", [(11025, 192000), (192000, 11025)])
def test_the_largest_bank_and_the_longest_span(sr, target):
    cfg = Resample.Config.create(sr, target)
    rng = np.random.default_rng(sr)
    for n in (1, 3001):
        x = rng.uniform(-1, 1, size=(3, n)).astype(np.float32)
        print(sr, target, n, "worst error / bound:", check_definition(cfg, x, Resample.apply(cfg, x)))


@pytest.mark.parametrize("sr,target,spec,n,why", [
    (8, 1, (200.0, 0.99), 20011, "K = 10700: the taps are staged in three chunks"),
    (100, 1, (40.0, 0.5), 50001, "M / L = 100: 64-output tiles"),
    (300, 1, (40.0, 0.5), 90001, "M / L = 300: no tile's input span fits LDS, samples read from global memory"),
])
def test_every_launch_plan(sr, target, spec, n, why):
    """the three ways the kernel is launched besides the common one (one tap chunk, 256-output tiles)"""
    cfg = Resample.Config.create(sr, target, Resample.Spec(*spec))
    assert cfg.executor == "direct"
    x = np.random.default_rng(n).uniform(-1, 1, size=(3, n)).astype(np.float32)
    print(why, "worst error / bound:", check_definition(cfg, x, Resample.apply(cfg, x)))


def test_positions_past_32_bits():
    """i M + K L passes 2^31 and 2^32 inside one clip (192000 -> 11025, M = 2560, 30 M samples): the outputs around both
    crossings and the last ones against the definition, evaluated here for those outputs alone."""
    import torch
    cfg = Resample.Config.create(192000, 11025)
    (l, m), k = cfg.rate, cfg.latency
    proto = cfg.prototype()
    n = 30_000_000
    gen = torch.Generator(device="cuda").manual_seed(7)
    x = torch.rand((1, n), device="cuda", generator=gen, dtype=torch.float32) * 2 - 1
    y = Resample.apply(cfg, x)
    n_out = -(-n * l // m)
    assert tuple(y.shape) == (1, n_out) and (n_out - 1) * m + k * l > 2 ** 32
    picks = []
    for edge in (2 ** 31, 2 ** 32):
        i = (edge - k * l) // m
        picks += list(range(i - 40, i + 40))
    picks += list(range(n_out - 80, n_out))
    xh = x[0].cpu().numpy().astype(np.float64)
    yh = y[0].cpu().numpy()
    j = np.arange(2 * k + 1)
    for i in picks:
        s = i * m + k * l
        p, q = s % l, s // l
        taps = np.zeros(2 * k + 1)
        col = proto[p::l]
        taps[:col.shape[0]] = col
        idx = q - j
        ok = (idx >= 0) & (idx < n)
        xv = np.where(ok, xh[np.clip(idx, 0, n - 1)], 0.0)
        want, scale = float(np.dot(taps, xv)), float(np.dot(np.abs(taps), np.abs(xv)))
        assert abs(float(yh[i]) - want) <= (2 * k + 3) * EPS * scale, (i, float(yh[i]), want)


# ---- 2. bit equalities ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sr,target", [(44100, 48000), (44100, 16000)])
def test_batch_host_device_and_strides_agree_bit_for_bit(sr, target):
    import torch
    cfg = Resample.Config.create(sr, target)
    rng = np.random.default_rng(11)
    n = 4999
    x = rng.uniform(-1, 1, size=(2, 3, n)).astype(np.float32)
    whole = Resample.apply(cfg, x)
    assert isinstance(whole, np.ndarray) and whole.shape == (2, 3, cfg.output_frames(n))
    for a in range(2):
        for b in range(3):
            assert np.array_equal(Resample.apply(cfg, x[a, b]), whole[a, b])          # the batch is its rows
    xd = torch.from_numpy(x).cuda()
    yd = Resample.apply(cfg, xd)
    assert yd.is_cuda and np.array_equal(yd.cpu().numpy(), whole)                     # host array = device tensor
    wide = torch.zeros((2, 3, n + 301), device="cuda")
    wide[..., 150:150 + n] = xd
    view = wide[..., 150:150 + n]
    assert not view.is_contiguous()
    assert np.array_equal(Resample.apply(cfg, view).cpu().numpy(), whole)             # a slice of a wider buffer = its copy
    assert np.array_equal(Resample.apply(cfg, xd[:, ::2]).cpu().numpy(), whole[:, ::2])
    assert np.array_equal(Resample.apply(cfg, xd.transpose(0, 1)).cpu().numpy(), whole.transpose(1, 0, 2))
    assert np.array_equal(Resample.apply(cfg, torch.from_numpy(x)).numpy(), whole)   # a CPU tensor comes back as one


@pytest.mark.parametrize("sr,target", [(48000, 16000), (16000, 48000)])
def test_the_overlap_save_classes_run_the_existing_stage(sr, target):
    cfg = Resample.Config.create(sr, target)
    assert cfg.executor == "ols"
    (l, m), k = cfg.rate, cfg.latency
    ks, fc, beta = M.single_stage(l, m)
    assert ks == k
    st = Resample.Stage.create(Resample.prototype(l, k, fc, beta), l, m, k)
    x = np.random.default_rng(3).uniform(-1, 1, size=(3, 23017)).astype(np.float32)
    assert np.array_equal(Resample.apply(cfg, x), Resample.Stage.apply(st, x))


def test_identity_flat_function_and_edges():
    import torch
    x = np.random.default_rng(4).uniform(-1, 1, size=(2, 1000)).astype(np.float32)
    ident = Resample.Config.create(48000, 48000)
    assert Resample.apply(ident, x) is x                                              # resample.mli:192-194
    xd = torch.from_numpy(x).cuda()
    assert Resample.apply(ident, xd) is xd
    cfg = Resample.Config.create(44100, 48000)
    assert np.array_equal(S.resample(x, 44100, 48000), Resample.apply(cfg, x))
    assert np.array_equal(S.resample(xd, 44100, 48000).cpu().numpy(), Resample.apply(cfg, x))
    fast = Resample.Config.create(44100, 48000, "fast")
    assert np.array_equal(S.resample(x, 44100, 48000, quality="fast"), Resample.apply(fast, x))
    assert S.resample(x, 44100, 48000, quality=S.Spec(100.0, 0.913)).shape == (2, 1089)
    assert Resample.apply(cfg, np.zeros((2, 0), dtype=np.float32)).shape == (2, 0)    # n = 0: empty
    assert tuple(Resample.apply(cfg, torch.zeros((2, 0), device="cuda")).shape) == (2, 0)
    with pytest.raises(S.InvalidArgument, match="rank-zero"):
        Resample.apply(cfg, np.float32(1.0))
    with pytest.raises(S.InvalidArgument, match="cannot resample float64 audio"):
        Resample.apply(cfg, x.astype(np.float64))
    with pytest.raises(S.InvalidArgument, match="cannot resample float64 audio"):
        Resample.apply(cfg, xd.double())


def test_more_channels_than_a_grid_dimension():
    """70000 channels in one call: the channel count is not capped by a grid dimension"""
    cfg = Resample.Config.create(5, 7)
    x = np.random.default_rng(6).uniform(-1, 1, size=(70000, 40)).astype(np.float32)
    y = Resample.apply(cfg, x)
    for c in (0, 65535, 65536, 69999):
        assert np.array_equal(y[c], Resample.apply(cfg, x[c]))
    check_definition(cfg, x[-3:], y[-3:])


# ---- 3. quality ----------------------------------------------------------------------------------------------------------

Q3_TONES = {(48000, 44100): (22700.0, 23200.0, 23520.0), (44100, 16000): (9000.0, 12000.0, 18000.0)}


@pytest.mark.parametrize("sr,target", [(44100, 48000), (48000, 44100), (44100, 16000)])
def test_config_meets_the_float32_thresholds(sr, target):
    cfg = Resample.Config.create(sr, target, "high")
    conv = lambda x: np.asarray(Resample.apply(cfg, f32(x)[None, :]))[0].astype(np.float64)
    nyq = min(sr, target) / 2.0
    report = []
    for frac in (0.045, 0.23, 0.45, 0.79):                      # Q1 / Q2
        mags = M.spectrum(conv(M.tone(sr, frac * nyq, 2.0)))
        report.append((frac, round(M.sfdr(mags), 1), round(M.thdn(mags), 1)))
    print(sr, target, "SFDR / THD+N:", report)
    for frac, d, t in report:
        assert d >= 125.0 and t <= -125.0, report
    for frac in (0.02, 0.5, 0.913):                              # Q4
        f = frac * nyq
        dev = abs(20.0 * np.log10(M.amp_at(target, f, conv(M.tone(sr, f, 1.0)))))
        print(sr, target, "Q4", frac, dev)
        assert dev <= 0.02, (frac, dev)
    for f in Q3_TONES.get((sr, target), ()):                     # Q3: out of band, under the input's own Nyquist
        assert f < sr / 2.0 and f > nyq
        peak = M.peak_dbfs(conv(M.tone(sr, f, 2.0)))
        print(sr, target, "Q3", f, peak)
        assert peak <= -125.0, (f, peak)


# ---- 4. streaming --------------------------------------------------------------------------------------------------------

CHUNKINGS = {
    "one": lambda n, rng: [0, n],
    "halves": lambda n, rng: [0, n // 2, n],
    "small": lambda n, rng: list(range(0, n, 97)) + [n],
    "random": lambda n, rng: [0] + sorted(set(int(v) for v in rng.integers(1, max(2, n), size=12))) + [n],
    "with_empty": lambda n, rng: [0, 0, n // 3, n // 3, n, n],
}
STREAMED = [(44100, 48000), (44100, 16000)]
N_STREAM = 23017


def ready(cfg, fed):
    (l, m), k = cfg.rate, cfg.latency
    return max(0, -(-(fed - k) * l // m))


def run(kern, cfg, x, cuts, flush_device=None):
    """every step, with the running total checked against `ready`; then flush"""
    parts, total = [], 0
    for a, b in zip(cuts[:-1], cuts[1:]):
        y = kern.step(x[..., a:b])
        if y is not None:
            assert y.shape[-1] > 0
            parts.append(y)
            total += int(y.shape[-1])
        assert total == ready(cfg, b), (a, b, total, ready(cfg, b))
    tail = kern.flush(device=flush_device) if flush_device else kern.flush()
    if tail is not None:
        parts.append(tail)
    assert kern.flush() is None                                  # a second flush has nothing
    return parts


_whole = {}


def signal_and_whole(sr, target):
    """one signal and one apply per ratio, shared by the streaming tests (read only)"""
    if (sr, target) not in _whole:
        cfg = Resample.Config.create(sr, target)
        x = np.random.default_rng(sr // 100 + target).uniform(-1, 1, size=(3, N_STREAM)).astype(np.float32)
        whole = Resample.apply(cfg, x)
        x.setflags(write=False)
        whole.setflags(write=False)
        _whole[(sr, target)] = (cfg, x, whole)
    return _whole[(sr, target)]


@pytest.mark.parametrize("chunking", sorted(CHUNKINGS))
@pytest.mark.parametrize("sr,target", STREAMED)
def test_partition_law(sr, target, chunking):
    cfg, x, whole = signal_and_whole(sr, target)
    rng = np.random.default_rng(len(chunking) + target)
    cuts = CHUNKINGS[chunking](N_STREAM, rng)
    kern = Resample.Kernel.prepare(cfg, channels=3, max_block=N_STREAM)
    parts = run(kern, cfg, x, cuts)
    assert all(isinstance(p, np.ndarray) for p in parts)
    got = np.concatenate(parts, axis=-1)
    assert got.shape == whole.shape == (3, cfg.output_frames(N_STREAM))
    assert np.array_equal(got, whole)
    kern.reset()                                                 # reset reproduces the first run
    again = np.concatenate(run(kern, cfg, x, cuts), axis=-1)
    assert np.array_equal(again, whole)


@pytest.mark.parametrize("sr,target", STREAMED)
def test_device_chunks_stay_on_the_device(sr, target):
    import torch
    cfg, x, whole = signal_and_whole(sr, target)
    cuts = [0, 5, 7000, 7001, 19000, N_STREAM]
    kern = Resample.Kernel.prepare(cfg, 3, N_STREAM)
    dev = run(kern, cfg, torch.from_numpy(np.array(x)).cuda(), cuts, flush_device="cuda")
    assert all(p.is_cuda for p in dev)
    assert np.array_equal(torch.cat(dev, dim=-1).cpu().numpy(), whole)


def test_short_streams_and_reset_mid_stream():
    cfg, x, whole = signal_and_whole(44100, 48000)
    k = cfg.latency
    kern = Resample.Kernel.prepare(cfg, 3, 4096)
    assert kern.step(x[:, :k]) is None                           # nothing is ready before K + 1 samples
    assert kern.flush().shape == (3, cfg.output_frames(k))       # ... and flush still emits the whole short signal
    kern.reset()
    assert kern.flush() is None                                  # an empty stream has no tail
    kern.reset()
    kern.step(x[:, :3000])
    kern.reset()                                                 # mid-stream: the history is zeroed
    parts = run(kern, cfg, x[:, :9000], [0, 4096, 8192, 9000])
    assert np.array_equal(np.concatenate(parts, axis=-1), Resample.apply(cfg, np.array(x[:, :9000])))


def test_stream_errors():
    cfg = Resample.Config.create(44100, 48000)
    with pytest.raises(S.InvalidArgument):
        Resample.Kernel.prepare(cfg, channels=0, max_block=16)
    with pytest.raises(S.InvalidArgument):
        Resample.Kernel.prepare(cfg, channels=1, max_block=0)
    kern = Resample.Kernel.prepare(cfg, channels=2, max_block=16)
    with pytest.raises(S.InvalidArgument, match="at most 16"):
        kern.step(np.zeros((2, 17), dtype=np.float32))           # longer than max_block
    with pytest.raises(S.InvalidArgument, match="2 channels"):
        kern.step(np.zeros((3, 4), dtype=np.float32))            # the wrong channel count
    kern.step(np.zeros((2, 4), dtype=np.float32))
    kern.flush()
    with pytest.raises(S.InvalidArgument, match="drained by flush"):
        kern.step(np.zeros((2, 4), dtype=np.float32))            # a step after flush
    kern.reset()
    assert kern.step(np.zeros((2, 4), dtype=np.float32)) is None


def test_ols_and_identity_configs_stream_too():
    x = np.random.default_rng(8).uniform(-1, 1, size=(2, 20000)).astype(np.float32)
    cfg = Resample.Config.create(48000, 16000)
    kern = Resample.Kernel.prepare(cfg, 2, 8192)
    parts = [kern.step(x[:, a:a + 8192]) for a in range(0, 20000, 8192)] + [kern.flush()]
    assert np.array_equal(np.concatenate([p for p in parts if p is not None], axis=-1), Resample.apply(cfg, x))
    ident = Resample.Kernel.prepare(Resample.Config.create(16000, 16000), 2, 8192)
    y = ident.step(x[:, :100])
    assert np.array_equal(y, x[:, :100]) and y is not x and not np.shares_memory(y, x)
    assert ident.flush() is None and ident.flush() is None
