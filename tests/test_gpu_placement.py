"""Placement: every device entry point on offset, padded, guarded buffers.

The other GPU tests hand the kernels fresh allocations: 512-byte aligned, packed rows, allocator slack on both sides of every
output.  Much of the hot path is dispatched on exactly these properties (8-byte aligned samples, even strides, the position of
the output pointer in its 128-byte line, 16-byte vector walks with scalar heads and tails), so here the same calls run on
buffers carved out of a guarded arena:

  * an arena is a flat int32 device tensor in which every word is S_PAD, a quiet NaN with a recognisable payload;
  * an input region holds rows of n elements, stride apart, from a chosen element offset on; whatever surrounds and separates
    the rows stays S_PAD, so a kernel that USES a sample outside a row poisons its result;
  * an output region is pre-filled with a second sentinel S_OUT; at least 128 words of S_PAD lie before and behind it, and the
    words that separate rows under an output stride are S_PAD too.

After the call (compared as int32 on the device): every guard word is still S_PAD, no output word is S_OUT (every element was
written), and the payload is (a) within the entry's existing gate of the float64 oracle and (b) bit for bit what the ordinary
call gives -- the same entry on the same data in fresh, aligned, packed buffers (placement (0, ..., 0) of the same helper).
Complex and float64 buffers move by whole elements: the element type's alignment is the ABI's contract.

TABLE names every `*_dev` entry point of include/soundml_amd.h that a row below runs; test_coverage_law fails for a new entry
point that is in neither TABLE nor EXCLUDED."""
import contextlib
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import soundml_amd as S
from soundml_amd import Chroma, Cqt, Effects, Fir, Hpss, Mel, Resample, Stft
from soundml_amd._lib import check, lib
from conftest import ROOT
from oracle import soundml_oracle as O
from oracle import resample_metrics as M

import cqt_restatement as CR
import effects_restatement as ER
import hpss_restatement as HR

pytestmark = pytest.mark.gpu

S_PAD = 0x7FF8DEAD      # a quiet NaN as float32, and as either half of a float64
S_OUT = 0x7FF8BEEF
GUARD = 128             # words before and behind every region: 512 bytes, so offset 0 is the allocator's own alignment
WORDS = {"float32": 1, "float64": 2, "complex64": 2, "complex128": 4}
INF = float("inf")

TABLE = {}              # entry point -> the tests that place it
EXCLUDED = {
    "smx_debug_stft_transform_frame_major_f32_dev": "diagnostic face (its layout is pinned by test_gpu_gl_frame_major.py)",
    "smx_debug_cqt_project_f32_dev": "diagnostic face (exact data in test_gpu_cqt.py)",
    "smx_stft_kernel_flush_dev": "runs at the end of the smx_stft_kernel_step_dev row",
    "smx_stft_synthesis_flush_dev": "runs at the end of the smx_stft_synthesis_step_dev row",
    "smx_cqt_kernel_flush_f32_dev": "runs at the end of the smx_cqt_kernel_step_f32_dev row",
    "smx_resample_kernel_flush_f32_dev": "runs at the end of the smx_resample_kernel_step_f32_dev row",
    "smx_resample_stream_flush_f32_dev": "runs at the end of the smx_resample_stream_step_f32_dev row",
    "smx_resample_shape_c128_dev": "three packed complex128 operands, no stride: its placement is fixed by test_gpu_host_faces.py",
}


def row(*entries):
    def mark(fn):
        for e in entries:
            TABLE.setdefault(e, []).append(fn.__name__)
        return fn
    return mark


@pytest.fixture(autouse=True)
def _default_interior():
    S.set_interior("float32")
    yield
    S.set_interior("float32")


# ---- the arena -------------------------------------------------------------------------------------------------------------

class Region:
    """rows of n elements of `dtype`, n + pad elements apart, the first one `off` elements behind a 512-byte aligned origin"""

    def __init__(self, rows, n, dtype, off=0, pad=0):
        import torch
        self.dtype = np.dtype(dtype)
        self.w = w = WORDS[self.dtype.name]
        self.rows, self.n, self.stride = int(rows), int(n), int(n) + int(pad)
        self.front = GUARD + off * w
        self.words = self.rows * self.stride * w
        self.buf = torch.full((self.front + self.words + GUARD,), S_PAD, dtype=torch.int32, device="cuda")
        assert self.buf.data_ptr() % 512 == 0
        self.ptr = C.c_void_p(self.buf.data_ptr() + 4 * self.front)
        self.output = False
        self.before = None

    def _rows(self, buf):
        return buf[self.front:self.front + self.words].view(self.rows, self.stride * self.w)

    @staticmethod
    def of(a, off=0, pad=None):
        """an input: the last axis of `a` is the row (pad: elements between rows), or, pad None, all of `a` is one packed row"""
        import torch
        a = np.ascontiguousarray(a)
        a = a.reshape(1, -1) if pad is None else a.reshape(-1, a.shape[-1])
        r = Region(a.shape[0], a.shape[1], a.dtype, off, pad or 0)
        r._rows(r.buf)[:, :r.n * r.w] = torch.tensor(a.view(np.int32).reshape(r.rows, r.n * r.w), device="cuda")
        r.before = r.buf.clone()
        return r

    @staticmethod
    def out(rows, n, dtype, off=0, pad=0):
        r = Region(rows, n, dtype, off, pad)
        r._rows(r.buf)[:, :r.n * r.w] = S_OUT
        r.output = True
        return r

    def intact(self):
        import torch
        assert torch.equal(self.buf, self.before), "an input buffer was written"

    def collect(self, used=None, tail_free=False):
        """the written payload as int32 [rows; used * w] once the guards and the sentinels have been checked; `used` < n: the
        call reported that many elements per row (tail_free: the rest of the row's capacity is the callee's to use)"""
        used = self.n if used is None else int(used)
        w = self.w
        assert 0 <= used <= self.n
        got = self._rows(self.buf)[:, :used * w].clone()
        unwritten = got == S_OUT
        assert not bool(unwritten.any()), "%d output words were never written, the first at %s" % (
            int(unwritten.sum()), unwritten.nonzero()[0].tolist())
        shadow = self.buf.clone()
        rows = self._rows(shadow)
        if self.output and not tail_free:
            assert bool((rows[:, used * w:self.n * w] == S_OUT).all()), "words behind the reported count were written"
        rows[:, :self.n * w] = S_PAD
        bad = shadow != S_PAD
        assert not bool(bad.any()), "%d guard words changed, the first at word %d of the region (rows of %d words, %d apart)" % (
            int(bad.sum()), int(bad.nonzero()[0]) - self.front, self.n * w, self.stride * w)
        return got


def host(bits, dtype, shape=None):
    a = np.ascontiguousarray(bits.cpu().numpy()).view(dtype)
    return a if shape is None else a.reshape(shape)


@contextlib.contextmanager
def environment(env):
    """the overrides the release build reads per call, put back as test_gpu_power32_shared_fetch._power does"""
    env = {k: v for k, v in (env or {}).items() if v is not None}
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def call(name, *args, env=None, inplace=False):
    import torch
    assert name in TABLE or name in EXCLUDED, name
    raw = [a.ptr if isinstance(a, Region) else a for a in args]
    with environment(env):
        check(getattr(lib, name)(*raw, C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        torch.cuda.synchronize()
    for a in args:
        if isinstance(a, Region) and not a.output and not inplace:
            a.intact()


def same(got, plain, what):
    import torch
    assert len(got) == len(plain)
    for k, (g, p) in enumerate(zip(got, plain)):
        if not torch.equal(g, p):
            d = (g != p).nonzero()
            raise AssertionError("%s: result %d differs from the ordinary call's in %d words, the first at %s" % (what, k, d.shape[0], d[0].tolist()))


def drive(run, placements, gate):
    """placements[0] is the ordinary call; every placement passes `gate` (the oracle) and equals the ordinary call bit for bit"""
    assert not any(placements[0])
    plain = run(placements[0])
    gate(plain, placements[0])
    for pl in placements[1:]:
        got = run(pl)
        gate(got, pl)
        same(got, plain, pl)
    return plain


def fast_gate(got, want, what):
    """test_gpu_parity.check_fast (|a - e| <= 1e-5 peak + 1e-5 |e|) per leading slice, complex values by their modulus"""
    assert got.shape == want.shape, (what, got.shape, want.shape)
    for a, e in zip(got, want):
        wide = np.complex128 if np.iscomplexobj(e) else np.float64
        d = np.abs(a.astype(wide) - e.astype(wide))
        peak = float(np.max(np.abs(e))) if e.size else 0.0
        bad = d > 1e-5 * peak + 1e-5 * np.abs(e)
        assert not bad.any(), "%s: %d/%d outside 1e-5 (max err %.3g, peak %.3g)" % (what, int(bad.sum()), d.size, float(d.max()), peak)


@functools.lru_cache(maxsize=None)
def signal(seed, clips, n):
    x = np.random.default_rng(seed).uniform(-1, 1, size=(clips, n)).astype(np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def configs(fft, hop):
    return Stft.Config.create(fft_size=fft, hop=hop), O.stft_config(fft, hop=hop)


@functools.lru_cache(maxsize=None)
def power_oracle(fft, hop, seed, clips, n, power):
    want = O.power_spectrum(configs(fft, hop)[1], signal(seed, clips, n).astype(np.float64), power)
    want.setflags(write=False)
    return want


@functools.lru_cache(maxsize=None)
def transform_oracle(fft, hop, seed, clips, n):
    want = O.transform(configs(fft, hop)[1], signal(seed, clips, n).astype(np.float64))
    want.setflags(write=False)
    return want


# ---- rows 1-3: smx_stft_power_range_f32_dev --------------------------------------------------------------------------------

def power_case(fft, hop, seed, clips, n, power, frame_range, envs, placements, peak_gate):
    """placements: (x_off, x_stride - n, out_off).  peak_gate: GATE * peak of the power32 files, else the north-star rule of
    test_gpu_power16 / test_gpu_power64"""
    c, _ = configs(fft, hop)
    x = signal(seed, clips, n)
    bins, frames = fft // 2 + 1, Stft.frames(c, n)
    p0, p1 = frame_range or (0, frames)
    want = power_oracle(fft, hop, seed, clips, n, power)[:, :, p0:p1]
    assert want.shape == (clips, bins, p1 - p0)
    peak = np.max(want, axis=(1, 2), keepdims=True)

    def gate(res, pl):
        got = host(res[0], np.float32, want.shape)
        if peak_gate:
            err = np.abs(got.astype(np.float64) - want)
            assert np.all(err <= 1e-5 * peak), (fft, n, power, frame_range, pl, float(np.max(err / peak)))
        else:
            fast_gate(got, want, (fft, n, power, pl))

    first = None
    for env in envs:
        def run(pl, env=env):
            x_off, x_pad, o_off = pl
            xin, out = Region.of(x, x_off, x_pad), Region.out(1, want.size, np.float32, o_off)
            call("smx_stft_power_range_f32_dev", c._h, xin, clips, n, n + x_pad, p0, p1, float(power), out, env=env)
            return [out.collect()]
        plain = drive(run, placements, gate)
        if first is None:
            first = plain
        same(plain, first, ("the ordinary call under", env))    # the switches select loads and stores, never arithmetic


@row("smx_stft_power_range_f32_dev")
@pytest.mark.parametrize("power", [2.0, 1.0, 0.7])
@pytest.mark.parametrize("frames", [48, 49])
def test_power_2048(frames, power):
    """row 1, stft2048_power32_kernel: 48 frames (shared span fetch where the samples are 8-byte aligned) and 49 (requests per
    half); an output offset of 1 or 31 takes the frame-per-lane flush (SKEW 2), 2 and 16 with an even pitch the pair flush
    (SKEW 1), SMX_POWER_SKEW=0 the plain flush; the range (1, 47) puts out_offset into `even`"""
    envs = [dict(SMX_FAST_BLOCKS=b, SMX_POWER_SKEW=s) for b in (None, "1") for s in (None, "0")]
    placements = [(0, 0, 0)] + [(xo, 0, oo) for xo in (0, 1) for oo in (1, 2, 16, 31)]
    for frame_range in (None, (1, 47)):
        power_case(2048, 512, 1, 3, 512 * (frames - 1), power, frame_range, envs, placements, True)


@row("smx_stft_power_range_f32_dev")
@pytest.mark.parametrize("fft,hop", [(1024, 256), (512, 128)])
def test_power_lanes(fft, hop):
    """row 2, stft_power_lanes_kernel<16 / 8>: one workgroup walks both clips, so the skewed flush of fft 1024 carries a row's
    trailing frames across tiles; 40 and 41 frames: both parities of the pitch"""
    envs = [dict(SMX_FAST_BLOCKS="1", SMX_POWER_SKEW=s) for s in (None, "0")]
    placements = [(0, 0, 0)] + [(0, 0, oo) for oo in (1, 2, 16, 31)]
    for frames in (40, 41):
        power_case(fft, hop, 2, 2, hop * (frames - 1), 2.0, None, envs, placements, False)


@row("smx_stft_power_range_f32_dev")
def test_power_256():
    """row 2, stft_power_lanes_kernel<4>: one case"""
    power_case(256, 64, 2, 2, 64 * 40, 2.0, None, [dict(SMX_FAST_BLOCKS="1")], [(0, 0, 0), (1, 0, 1)], False)


@row("smx_stft_power_range_f32_dev")
@pytest.mark.parametrize("frames", [33, 34])
def test_power_4096(frames):
    """row 3, stft4096_power64_kernel<ALIGNED, power, EVEN>: both parities of out_stride, the pointer 4 and 8 bytes off"""
    placements = [(0, 0, 0)] + [(xo, 0, oo) for xo in (0, 1) for oo in (1, 2)]
    power_case(4096, 1024, 3, 2, 1024 * (frames - 1), 2.0, None, [None], placements, False)


# ---- row 4: smx_stft_transform_range_f32_dev -------------------------------------------------------------------------------

@row("smx_stft_transform_range_f32_dev")
@pytest.mark.parametrize("fft,hop,n", [(2048, 512, 512 * 39), (1024, 256, 256 * 39), (100, 33, 37 * 33 + 55)])
def test_transform(fft, hop, n):
    """stft2048_complex32_kernel<ALIGNED, CSKEW> (the line flush needs an 8-byte aligned origin: any whole complex element),
    stft_complex_lanes_kernel<16>, and the generic route; offsets of 1 and 8 complex elements: 8 and 64 bytes into a line"""
    c, _ = configs(fft, hop)
    clips, seed = 2, 4
    x = signal(seed, clips, n)
    want = transform_oracle(fft, hop, seed, clips, n)
    frames = want.shape[-1]
    assert frames == Stft.frames(c, n)
    placements = [(0, 0, 0)] + [(xo, xp, oo) for xo in (0, 1) for xp in (1, 6) for oo in (1, 8)]
    first = None
    for skew in (None, "0"):
        def run(pl):
            x_off, x_pad, o_off = pl
            xin, out = Region.of(x, x_off, x_pad), Region.out(1, want.size, np.complex64, o_off)
            call("smx_stft_transform_range_f32_dev", c._h, xin, clips, n, n + x_pad, 0, frames, out, env=dict(SMX_COMPLEX_SKEW=skew))
            return [out.collect()]
        plain = drive(run, placements, lambda res, pl: fast_gate(host(res[0], np.complex64, want.shape), want, (fft, pl)))
        first = first or plain
        same(plain, first, "SMX_COMPLEX_SKEW=0")


# ---- row 5: the float64 faces ----------------------------------------------------------------------------------------------

@row("smx_stft_transform_range_f64_dev", "smx_stft_power_range_f64_dev")
def test_float64_faces():
    """fft 512 / hop 128 on the Stockham passes in doubles (test_float64_interior_stockham_sizes and its tolerances)"""
    fft, hop = 512, 128
    c, o = configs(fft, hop)
    x = np.random.default_rng(5).standard_normal((2, 9 * fft + 123))
    clips, n = x.shape
    frames = Stft.frames(c, n)
    wz, wp = O.transform(o, x), O.power_spectrum(o, x, 1.0)
    scale = float(np.max(np.abs(wz)))
    placements = [(0, 0, 0), (1, 1, 1)]

    def run_z(pl):
        xin, out = Region.of(x, pl[0], pl[1]), Region.out(1, wz.size, np.complex128, pl[2])
        call("smx_stft_transform_range_f64_dev", c._h, xin, clips, n, n + pl[1], 0, frames, out)
        return [out.collect()]

    def run_p(pl):
        xin, out = Region.of(x, pl[0], pl[1]), Region.out(1, wp.size, np.float64, pl[2])
        call("smx_stft_power_range_f64_dev", c._h, xin, clips, n, n + pl[1], 0, frames, 1.0, out)
        return [out.collect()]
    drive(run_z, placements, lambda res, pl: np.testing.assert_allclose(host(res[0], np.complex128, wz.shape), wz, rtol=1e-9, atol=1e-12 * scale))
    drive(run_p, placements, lambda res, pl: np.testing.assert_allclose(host(res[0], np.float64, wp.shape), wp, rtol=1e-9, atol=1e-12 * scale))


# ---- row 6: the fused features ---------------------------------------------------------------------------------------------

FEATURE_PLACEMENTS = [(0, 0, 0)] + [(xo, 3, oo) for xo in (0, 1) for oo in (1, 3)]


@row("smx_mel_spectrogram_f32_dev", "smx_mfcc_f32_dev", "smx_chroma_stft_f32_dev")
@pytest.mark.parametrize("fft,hop", [(2048, 512), (1024, 256)])
def test_fused_features(fft, hop):
    """stft2048_mel32_kernel / stft_mel_lanes_kernel<16> under `aligned` and not; mfcc adds mel_max_kernel and the DCT tail,
    chroma_stft the power kernel into scratch and the projection"""
    sr, clips, n = 22050, 2, hop * 39
    c, o = configs(fft, hop)
    x = signal(6, clips, n)
    frames = Stft.frames(c, n)
    assert frames == 40
    mc, omc = Mel.Config.create(n_mels=40, sample_rate=sr, fft_size=fft), O.mel_config(40, sr, fft)
    cc, occ = Chroma.Config.create(sr, fft), O.chroma_config(sr, fft)
    kind, p = Chroma.norm_args("inf")
    want_mel = O.mel_spectrogram(o, omc, x)
    want_mfcc = O.mfcc(o, omc, x, 13, None)
    want_chroma = O.chroma_stft(o, occ, x)
    assert want_mel.shape == (clips, 40, frames) and want_mfcc.shape == (clips, 13, frames) and want_chroma.shape == (clips, 12, frames)

    def runner(entry, size, before, after):
        def run(pl):
            xin, out = Region.of(x, pl[0], pl[1]), Region.out(1, size, np.float32, pl[2])
            call(entry, *before, xin, clips, n, n + pl[1], *after, out)
            return [out.collect()]
        return run
    drive(runner("smx_mel_spectrogram_f32_dev", want_mel.size, (c._h, mc._h), (2.0,)), FEATURE_PLACEMENTS,
          lambda res, pl: fast_gate(host(res[0], np.float32, want_mel.shape), want_mel, ("mel", fft, pl)))
    drive(runner("smx_mfcc_f32_dev", want_mfcc.size, (c._h, mc._h), (13, 0, 0.0)), FEATURE_PLACEMENTS,     # test_mfcc_vs_oracle_batch
          lambda res, pl: np.testing.assert_allclose(host(res[0], np.float32, want_mfcc.shape), want_mfcc, rtol=1e-4, atol=2e-3))
    drive(runner("smx_chroma_stft_f32_dev", want_chroma.size, (c._h, cc._h), (2.0, kind, p)), FEATURE_PLACEMENTS,   # test_chroma_stft_vs_oracle_c2_geometry
          lambda res, pl: np.testing.assert_allclose(host(res[0], np.float32, want_chroma.shape), want_chroma, rtol=1e-5, atol=1e-5))


# ---- row 7: decibels -------------------------------------------------------------------------------------------------------

DB = {"smx_power_to_db_f32_dev": O.power_to_db, "smx_amplitude_to_db_f32_dev": O.amplitude_to_db}
LOUD, QUIET = np.float32(1e6), np.float32(1e-9)     # the unique maximum; a value 150 dB under it, which must clamp


def db_values(total, top, nan_head=False):
    """the data of test_db_vs_oracle_large at size `total`; top: where the unique maximum sits (None: no clamp), with a value
    that must clamp at each of the other two of (head, middle, tail)"""
    rng = np.random.default_rng(7 * total + (top or 0))
    s = (rng.standard_normal(total) * np.exp(rng.uniform(-20, 5, size=total))).astype(np.float32)
    if top is not None:
        for place in {0, total // 2, total - 1}:
            s[place] = QUIET
        s[top] = LOUD
    if nan_head:
        s[0] = np.nan
    return s


def db_case(entry, s, top_db):
    total = s.size
    want = DB[entry](s, reference=2.0, top_db=top_db)
    args = (total, 2.0, 1e-10 if "power" in entry else 1e-5, 0 if top_db is None else 1, 0.0 if top_db is None else top_db)

    def run(pl):
        s_off, o_off = pl
        sin = Region.of(s, s_off)
        if o_off is None:       # in place: every element is read and written by the same lane
            call(entry, sin, *args, sin, inplace=True)
            return [sin.collect()]
        out = Region.out(1, total, np.float32, o_off)
        call(entry, sin, *args, out)
        return [out.collect()]
    # s_off: the head of the peeled walk holds (4 - s_off) % 4 elements; o_off == s_off: the vector walk; s_off + 1, + 2: the
    # all-scalar walk (s and out differ mod 16 bytes)
    placements = [(0, 0)] + [(so, oo) for so in (0, 1, 2, 3) for oo in (so, so + 1, so + 2, None) if (so, oo) != (0, 0)]
    drive(run, placements, lambda res, pl: np.testing.assert_allclose(host(res[0], np.float32, want.shape), want, rtol=2e-6, atol=2e-4,
                                                                      err_msg="%s total %d top_db %s %s" % (entry, total, top_db, pl)))


@row("smx_power_to_db_f32_dev", "smx_amplitude_to_db_f32_dev")
@pytest.mark.parametrize("total", [1, 3, 5, 4099])
@pytest.mark.parametrize("entry", sorted(DB))
def test_to_db(entry, total):
    """to_db_kernel's head / vector / tail walks and its scalar walk, db_max_kernel's head and tail: the tensor's maximum in the
    head, in the tail and mid-vector (tolerances of test_db_vs_oracle_large)"""
    db_case(entry, db_values(total, None), None)
    for top in sorted({0, total // 2, total - 1}):
        s = db_values(total, top)
        if total > 1:
            assert np.sum(s == LOUD) == 1 and np.sum(np.abs(s) >= LOUD) == 1
        db_case(entry, s, 80.0)


@row("smx_power_to_db_f32_dev", "smx_amplitude_to_db_f32_dev")
@pytest.mark.parametrize("entry", sorted(DB))
def test_to_db_nan_in_the_head(entry):
    """a NaN stays a NaN, and as the tensor's maximum it makes every clamped value one (Nx.maximum leaves it)"""
    for top_db in (None, 80.0):
        db_case(entry, db_values(4099, None, nan_head=True), top_db)


# ---- row 8: spectrogram-domain entries -------------------------------------------------------------------------------------

PLANE = (2, 257, 37)
PLANE_PLACEMENTS = [(0, 0)] + [(i, o) for i in (1, 3) for o in (1, 3)]


def plane_call(entry, s, outs, before, after, dtype=np.float32):
    """entry(before..., s, lead, bins, frames, after..., outs...) with the spectrogram `off` elements in and every result
    `o_off` elements in; outs: the shapes of the results"""
    lead, bins, frames = s.shape

    def run(pl):
        sin = Region.of(s, pl[0])
        regions = [Region.out(1, int(np.prod(shape)), dtype, pl[1]) for shape in outs]
        call(entry, *before, sin, lead, bins, frames, *after, *regions)
        return [r.collect() for r in regions]
    return run


@row("smx_mel_apply_f32_dev", "smx_mel_apply_f64_dev", "smx_chroma_apply_f32_dev")
def test_projections():
    """mel_apply (float32 and float64) and chroma_apply at 2 x 257 x 37: an odd frame count, so every row of every clip starts
    at another position of its 16-byte group"""
    rng = np.random.default_rng(8)
    s64 = rng.uniform(0, 4, size=PLANE)
    s32 = s64.astype(np.float32)
    mc, omc = Mel.Config.create(n_mels=40, sample_rate=22050, fft_size=512), O.mel_config(40, 22050, 512)
    for s, entry, dtype in ((s32, "smx_mel_apply_f32_dev", np.float32), (s64, "smx_mel_apply_f64_dev", np.float64)):
        want = O.mel_apply(omc, s)

        def gate(res, pl, want=want, dtype=dtype):      # test_mel_apply_vs_oracle
            got = host(res[0], dtype, want.shape)
            if dtype == np.float64:
                np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-14)
            else:
                fast_gate(got, want, ("mel_apply", pl))
        drive(plane_call(entry, s, [want.shape], (mc._h,), (), dtype), PLANE_PLACEMENTS, gate)
    cc, occ = Chroma.Config.create(22050, 512), O.chroma_config(22050, 512)
    sq = (rng.standard_normal(PLANE) ** 2).astype(np.float32)
    sq[1, :, 5] = 0.0
    want = O.chroma_apply(occ, sq, norm="inf")
    kind, p = Chroma.norm_args("inf")
    drive(plane_call("smx_chroma_apply_f32_dev", sq, [want.shape], (cc._h,), (kind, p)), PLANE_PLACEMENTS,     # test_chroma_apply_vs_oracle
          lambda res, pl: np.testing.assert_allclose(host(res[0], np.float32, want.shape), want, rtol=2e-6, atol=2e-6 * float(np.max(np.abs(want)))))


@row("smx_spectral_centroid_f32_dev", "smx_spectral_bandwidth_f32_dev", "smx_spectral_rolloff_f32_dev", "smx_spectral_flatness_f32_dev")
def test_spectral():
    """the four bin-axis reductions (tolerances of test_spectral_vs_oracle); bandwidth also with the caller's centroid offset"""
    rng = np.random.default_rng(sum(PLANE))
    s = np.abs(rng.standard_normal(PLANE)).astype(np.float32)
    s[..., :, 0] = 0.0
    lead, bins, frames = PLANE
    shape = (lead, 1, frames)
    sr = 22050

    def close(want, exact=False):
        def gate(res, pl):
            got = host(res[0], np.float32, shape)
            if exact:
                assert np.mean(got == want) >= 0.999, pl
            else:
                np.testing.assert_allclose(got, want, rtol=2e-6, atol=1e-7 * float(np.max(want)), err_msg=str(pl))
        return gate
    drive(plane_call("smx_spectral_centroid_f32_dev", s, [shape], (), (None, 0, sr)), PLANE_PLACEMENTS, close(O.spectral_centroid(s, sample_rate=sr)))
    drive(plane_call("smx_spectral_bandwidth_f32_dev", s, [shape], (), (2.0, None, 0, None, 0, 0, sr)), PLANE_PLACEMENTS,
          close(O.spectral_bandwidth(s, sample_rate=sr)))
    drive(plane_call("smx_spectral_rolloff_f32_dev", s, [shape], (), (0.85, None, 0, sr)), PLANE_PLACEMENTS,
          close(O.spectral_rolloff(s, sample_rate=sr), exact=True))
    drive(plane_call("smx_spectral_flatness_f32_dev", s, [shape], (), (1e-10, 2.0)), PLANE_PLACEMENTS, close(O.spectral_flatness(s)))
    centroid = S.spectral_centroid(s, sample_rate=sr)
    assert centroid.shape == shape and centroid.dtype == np.float32

    def run(pl):
        sin, cin, out = Region.of(s, pl[0]), Region.of(centroid, pl[2]), Region.out(1, lead * frames, np.float32, pl[1])
        call("smx_spectral_bandwidth_f32_dev", sin, lead, bins, frames, 2.0, None, 0, cin, 1, frames, sr, out)
        return [out.collect()]
    drive(run, [(0, 0, 0), (1, 3, 1), (3, 1, 3), (0, 0, 1)], close(O.spectral_bandwidth(s, sample_rate=sr, centroid=centroid)))


@row("smx_hpss_masks_f32_dev", "smx_hpss_of_spectrogram_f32_dev", "smx_hpss_of_stft_c64_dev")
def test_hpss_planes():
    """the median filters and the masks against the restatement, with test_gpu_hpss's rules: hard masks without a flipped cell,
    the soft product within one ulp, the complex face within 1e-6 |e| + 1e-7 peak"""
    from test_gpu_hpss import plane_stack, ulp_distance
    kernel, margin = (17, 31), (1.0, 1.0)
    s = plane_stack(PLANE, 11)
    harm, perc = HR.medians(s, kernel)
    params = (kernel[0], kernel[1])

    def hard(res, pl):
        want = HR.softmask(harm, perc, INF, True), HR.softmask(perc, harm, INF, True)
        assert sum(int((host(r, np.float32, PLANE) != w).sum()) for r, w in zip(res, want)) == 0, pl
    drive(plane_call("smx_hpss_masks_f32_dev", s, [PLANE, PLANE], (), params + (INF,) + margin), PLANE_PLACEMENTS, hard)

    def soft(res, pl):
        want = s * HR.softmask(harm, perc, 2.0, True), s * HR.softmask(perc, harm, 2.0, True)
        assert max(int(ulp_distance(host(r, np.float32, PLANE), w).max()) for r, w in zip(res, want)) <= 1, pl
    drive(plane_call("smx_hpss_of_spectrogram_f32_dev", s, [PLANE, PLANE], (), params + (2.0,) + margin), PLANE_PLACEMENTS, soft)
    rng = np.random.default_rng(12)
    z = (rng.standard_normal(PLANE) + 1j * rng.standard_normal(PLANE)).astype(np.complex64)
    want_z = HR.hpss_of_stft(z, kernel, 2.0, margin)

    def cplx(res, pl):
        for r, e in zip(res, want_z):
            a = host(r, np.complex64, PLANE)
            peak = float(np.max(np.abs(e)))
            assert float(np.max(np.abs(a - e) - (1e-6 * np.abs(e) + 1e-7 * peak))) <= 0.0, pl
    drive(plane_call("smx_hpss_of_stft_c64_dev", z, [PLANE, PLANE], (), params + (2.0,) + margin, np.complex64), [(0, 0), (1, 1)], cplx)


# ---- row 9: synthesis ------------------------------------------------------------------------------------------------------

def random_spectrum(seed, lead, bins, frames, dtype):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((lead, bins, frames)) + 1j * rng.standard_normal((lead, bins, frames))).astype(dtype)


def invert_case(entry, fft, hop, frames, lengths, placements, envs, wide=False):
    """placements: (z_off in complex elements, out_off)"""
    c, o = configs(fft, hop)
    lead, bins = 2, fft // 2 + 1
    z = random_spectrum(fft + hop, lead, bins, frames, np.complex128 if wide else np.complex64)
    real = np.float64 if wide else np.float32
    for length in lengths:
        want = O.invert(o, z, length)
        out_len = want.shape[-1]

        def gate(res, pl):
            got = host(res[0], real, want.shape)
            if wide:
                np.testing.assert_allclose(got, want, rtol=1e-9, atol=1e-11)       # test_invert_vs_oracle
            else:
                fast_gate(got[None], want[None], (fft, length, pl))                 # (check_fast over the whole result, as there)
        for env in envs:
            def run(pl, env=env):
                zin, out = Region.of(z, pl[0]), Region.out(1, lead * out_len, real, pl[1])
                call(entry, c._h, zin, lead, bins, frames, 0 if length is None else 1, length or 0, out, env=env)
                return [out.collect()]
            drive(run, placements, gate)


@row("smx_stft_invert_f32_dev")
def test_invert_2048():
    """istft pipeline kernel and, SMX_INVERT_PIPELINE=0, the tile kernel: `aligned_out` true and false at an even and an odd
    length (the second clip starts on the other parity when the length is odd)"""
    default = 512 * 39
    placements = [(0, 0)] + [(zo, oo) for zo in (0, 1) for oo in (0, 1, 2) if (zo, oo) != (0, 0)]
    invert_case("smx_stft_invert_f32_dev", 2048, 512, 40, (default, default - 1), placements, [None, dict(SMX_INVERT_PIPELINE="0")])


@row("smx_stft_invert_f32_dev", "smx_stft_invert_f64_dev")
def test_invert_other_routes():
    """the fused quarter-hop kernel at fft 1024, a generic size, and the float64 face"""
    invert_case("smx_stft_invert_f32_dev", 1024, 256, 40, (None,), [(0, 0), (1, 1), (1, 2)], [None])
    invert_case("smx_stft_invert_f32_dev", 100, 25, 23, (None, 501), [(0, 0), (1, 1)], [None])
    invert_case("smx_stft_invert_f64_dev", 512, 128, 23, (None,), [(0, 0), (1, 1)], [None], wide=True)


@row("smx_stft_griffin_lim_f32_dev")
def test_griffin_lim():
    """two iterations of the fused loop at fft 2048 (tolerances of test_griffin_lim_folded_update_short_runs)"""
    c, o = configs(2048, 512)
    x = signal(9, 2, 512 * 39)
    mag = np.abs(Stft.transform(c, x)).astype(np.float32)
    lead, bins, frames = mag.shape
    want = O.griffin_lim(o, mag, 2, 0.99, None, None)
    peak = np.max(np.abs(want))

    def gate(res, pl):
        got = host(res[0], np.float32, want.shape)
        assert np.max(np.abs(got - want)[:, 2048:-2048]) < 2e-4 * peak, pl
        assert np.linalg.norm(got - want) < 1e-3 * np.linalg.norm(want), pl

    def run(pl):
        sin, out = Region.of(mag, pl[0]), Region.out(1, want.size, np.float32, pl[1])
        call("smx_stft_griffin_lim_f32_dev", c._h, sin, lead, bins, frames, 2, 0.99, None, 0, 0, out)
        return [out.collect()]
    drive(run, [(0, 0), (1, 1)], gate)


# ---- row 10: effects and the signal face of hpss ---------------------------------------------------------------------------

@row("smx_phase_vocoder_c64_dev", "smx_phase_vocoder_c128_dev")
@pytest.mark.parametrize("phase", ["independent", "locked"])
def test_phase_vocoder(phase):
    """fft 64 / hop 16 / 9 frames of test_gpu_effects against the restatement, at its bounds"""
    fft, hop, frames, rate, lead = 64, 16, 9, 1.37, 3
    bins = fft // 2 + 1
    c = Stft.Config.create(fft_size=fft, hop=hop, pad=("constant", 0.0))
    z128 = random_spectrum(10, lead, bins, frames, np.complex128)
    count = Effects.out_frames(frames, rate)
    for entry, z in (("smx_phase_vocoder_c64_dev", z128.astype(np.complex64)), ("smx_phase_vocoder_c128_dev", z128)):
        want = ER.vocode(fft, hop, z, rate, locked=phase == "locked").astype(z.dtype)
        assert want.shape == (lead, bins, count)
        peak = float(np.max(np.abs(want)))
        bound = 2.0 ** -22 * peak if z.dtype == np.complex64 else 1e-11 * max(1.0, peak)

        def gate(res, pl, want=want, bound=bound):
            got = host(res[0], want.dtype, want.shape)
            assert float(np.max(np.abs(got.astype(np.complex128) - want.astype(np.complex128)))) <= bound, pl

        def run(pl, entry=entry, z=z, want=want):
            zin, out = Region.of(z, pl[0]), Region.out(1, want.size, z.dtype, pl[1])
            call(entry, c._h, zin, lead, bins, frames, rate, 1 if phase == "locked" else 0, out)
            return [out.collect()]
        drive(run, [(0, 0), (1, 1)], gate)


@row("smx_time_stretch_f32_dev", "smx_pitch_shift_f32_dev", "smx_hpss_f32_dev")
def test_signal_effects():
    """each is, bit for bit, the composition of its stages (test_gpu_effects, test_gpu_hpss.test_composition_law), which the
    rows above compare with the oracle one by one"""
    import torch
    fft, hop, n, lead = 256, 64, 4000, 2
    c = Stft.Config.create(fft_size=fft, hop=hop, pad=("constant", 0.0))
    x = signal(11, lead, n)
    xd = torch.from_numpy(np.array(x)).cuda()
    bits = lambda t: t.contiguous().view(torch.int32).reshape(1, -1)
    rate = 0.75
    length = ER.stretch_length(n, rate)
    staged = Stft.invert(c, Effects.phase_vocoder(c, Stft.transform(c, xd), rate), length=length)

    def stretch(pl):
        xin, out = Region.of(x, pl[0]), Region.out(1, lead * length, np.float32, pl[1])
        call("smx_time_stretch_f32_dev", c._h, xin, lead, n, rate, 0, out)
        return [out.collect()]
    drive(stretch, [(0, 0), (1, 1)], lambda res, pl: same(res, [bits(staged)], ("time_stretch stages", pl)))
    num, den = 3, 2
    r = Resample.Config.create(num, den)
    y = Resample.apply(r, Effects.time_stretch(c, xd, float(den) / float(num)))
    shifted = torch.zeros((lead, n), dtype=torch.float32, device="cuda")
    kept = min(n, int(y.shape[-1]))
    shifted[:, :kept] = y[:, :kept]

    def shift(pl):
        xin, out = Region.of(x, pl[0]), Region.out(1, lead * n, np.float32, pl[1])
        call("smx_pitch_shift_f32_dev", c._h, r._h, 0, xin, lead, n, out)
        return [out.collect()]
    drive(shift, [(0, 0), (1, 1)], lambda res, pl: same(res, [bits(shifted)], ("pitch_shift stages", pl)))
    c2, _ = configs(2048, 512)
    n2 = 6000
    x2 = signal(12, lead, n2)
    x2d = torch.from_numpy(np.array(x2)).cuda()
    kw = dict(kernel_size=(17, 31), power=2.0, margin=(1.0, 2.0))
    z_h, z_p = Hpss.hpss_of_stft(Stft.transform(c2, x2d), **kw)
    w_h, w_p = Stft.invert(c2, z_h, length=n2), Stft.invert(c2, z_p, length=n2)

    def separate(pl):
        xin = Region.of(x2, pl[0])
        y_h, y_p = Region.out(1, lead * n2, np.float32, pl[1]), Region.out(1, lead * n2, np.float32, pl[1])
        call("smx_hpss_f32_dev", c2._h, xin, lead, n2, 17, 31, 2.0, 1.0, 2.0, y_h, y_p)
        return [y_h.collect(), y_p.collect()]
    drive(separate, [(0, 0), (1, 1)], lambda res, pl: same(res, [bits(w_h), bits(w_p)], ("hpss stages", pl)))


# ---- rows 11 and 12: FIR and the resampler ---------------------------------------------------------------------------------

ROWS_PLACEMENTS = [(0, 0, 0, 0), (0, 0, 1, 1), (0, 0, 2, 4), (1, 0, 0, 0), (0, 1, 0, 0), (1, 1, 1, 3)]      # (x_off, y_off, x_stride - n, y_stride - n)


def rows_call(entry, handle, x, n_out):
    channels, n = x.shape

    def run(pl):
        x_off, y_off, x_pad, y_pad = pl
        xin, out = Region.of(x, x_off, x_pad), Region.out(channels, n_out, np.float32, y_off, y_pad)
        call(entry, handle, xin, channels, n, n + x_pad, out, n_out + y_pad)
        return [out.collect()]
    return run


@row("smx_fir_apply_f32_dev")
@pytest.mark.parametrize("taps,block", [(63, 0), (200, 1024), (400, 2048), (600, 4096), (1500, 8192), (3000, 16384), (8192, 32768)])
def test_fir(taps, block):
    """fir_direct_kernel (16-byte or scalar stores per address), fir_ols_real_kernel<9 .. 13, ALIGNED> and fir_ols_pk32_kernel<ALIGNED>:
    two whole blocks and a ragged one; n is odd, so (0, 0, 1, 1) is the aligned form over padded rows, (0, 0, 2, 4) the
    element-wise one with differing strides, and a pointer 4 bytes off with packed odd rows the element-wise form again"""
    h = Fir.design_lowpass(taps, 0.25, 80.0)
    plan = Fir.Plan.create(h)
    if block:
        assert plan.block == block
    step = block - (taps & ~1) if block else 2048     # fir.hip: the block advance N - lead; the direct kernel's tile
    n = 2 * step + 1001
    x = signal(taps, 2, n)
    want = O.fir_filter(h, x)
    bound = 1e-5 * np.sum(np.abs(h)) * np.max(np.abs(x))           # test_fir_vs_oracle
    placements = ROWS_PLACEMENTS + ([] if block else [(0, 2, 0, 0), (0, 3, 0, 0), (2, 1, 0, 0)])
    drive(rows_call("smx_fir_apply_f32_dev", plan._h, x, n), placements,
          lambda res, pl: np.max(np.abs(host(res[0], np.float32, want.shape).astype(np.float64) - want)) <= bound or pytest.fail("%s: outside 1e-5 sum|h| max|x|" % (pl,)))


RESAMPLE_PLACEMENTS = [(0, 0, 0, 0), (0, 0, 1, 1), (1, 1, 1, 3), (0, 0, 2, 4)]


@row("smx_resample_stage_apply_f32_dev")
@pytest.mark.parametrize("l,m,k", [(2, 1, 160), (1, 2, 161), (3, 2, 60)])
def test_resample_stage(l, m, k):
    """the polyphase-block stage (x2, /2) and the block convolution at the interpolated rate (3/2) (test_resample_stage_vs_oracle)"""
    n = 20001
    proto = Resample.prototype(l, k, 0.45 / max(l, m), O.kaiser_beta(100.0))
    st = Resample.Stage.create(proto, l, m, k)
    x = signal(100 * l + m, 2, n)
    want = O.resample_stage_direct(proto, l, m, k, x.astype(np.float64))
    n_out = -(-n * l // m)
    assert want.shape == (2, n_out)
    bound = 1e-5 * np.sum(np.abs(proto))
    drive(rows_call("smx_resample_stage_apply_f32_dev", st._h, x, n_out), RESAMPLE_PLACEMENTS,
          lambda res, pl: np.max(np.abs(host(res[0], np.float32, want.shape).astype(np.float64) - want)) <= bound or pytest.fail("%s: outside 1e-5 sum|proto|" % (pl,)))


@row("smx_resample_apply_f32_dev")
def test_resample_apply():
    """the direct polyphase executor at 5 -> 7 (test_gpu_resample_config.check_definition: (2 K + 3) eps of the absolute sum)"""
    cfg = Resample.Config.create(5, 7)
    assert cfg.executor == "direct"
    (l, m), k = cfg.rate, cfg.latency
    proto = cfg.prototype()
    n = 5001
    x = signal(57, 2, n)
    n_out = cfg.output_frames(n)
    want = np.stack([M.stage_polyphase(proto, l, m, k, r) for r in x])
    tol = (2 * k + 3) * 2.0 ** -24 * np.stack([M.stage_polyphase(np.abs(proto), l, m, k, np.abs(r)) for r in x])

    def gate(res, pl):
        assert np.all(np.abs(host(res[0], np.float32, want.shape).astype(np.float64) - want) <= tol), pl
    drive(rows_call("smx_resample_apply_f32_dev", cfg._h, x, n_out), RESAMPLE_PLACEMENTS, gate)


# ---- row 13: constant-Q ----------------------------------------------------------------------------------------------------

CQT_PLACEMENTS = [(0, 0, 0)] + [(xo, 5, 1) for xo in (0, 1)]


@row("smx_cqt_transform_f32_dev", "smx_cqt_power_spectrum_f32_dev", "smx_chroma_cqt_f32_dev", "smx_chroma_of_cqt_f32_dev")
def test_cqt():
    """n_bins 7 (one octave behind six early decimations), the smallest plan of test_gpu_cqt: the transform against the
    restatement at 5e-6 of the peak, the magnitude exactly from the rounded transform, chroma_cqt exactly its two steps, and
    the fold alone against the restatement at chroma_apply's tolerance"""
    import torch
    from test_gpu_cqt import device_decimate
    kw = dict(n_bins=7, sample_rate=22050)
    c, r = Cqt.Config.create(**kw), CR.Config(**kw)
    lead, n = 2, 8192
    x = signal(13, lead, n)
    frames = Cqt.frames(c, n)
    want = CR.transform(r, x.astype(np.float64), device_decimate)
    assert want.shape == (lead, 7, frames)
    peak = float(np.max(np.abs(want)))

    def runner(entry, size, dtype, after):
        def run(pl):
            xin, out = Region.of(x, pl[0], pl[1]), Region.out(1, size, dtype, pl[2])
            call(entry, c._h, xin, lead, n, n + pl[1], *after, out)
            return [out.collect()]
        return run
    zbits = drive(runner("smx_cqt_transform_f32_dev", want.size, np.complex64, ()), CQT_PLACEMENTS,
                  lambda res, pl: float(np.max(np.abs(host(res[0], np.complex64, want.shape).astype(np.complex128) - want))) <= CR.TIGHT32_ATOL * peak
                  or pytest.fail("%s: outside 5e-6 of the peak" % (pl,)))
    z = host(zbits[0], np.complex64, want.shape)
    mag = np.sqrt(z.real.astype(np.float64) ** 2 + z.imag.astype(np.float64) ** 2).astype(np.float32)
    drive(runner("smx_cqt_power_spectrum_f32_dev", mag.size, np.float32, (1.0,)), CQT_PLACEMENTS,
          lambda res, pl: np.array_equal(host(res[0], np.float32, mag.shape), mag) or pytest.fail("%s: not |transform|" % (pl,)))
    kind, p = Chroma.norm_args("inf")
    two_steps = Chroma.of_cqt(c, torch.from_numpy(mag).cuda(), n_chroma=12, norm="inf")
    bits = two_steps.contiguous().view(torch.int32).reshape(1, -1)
    drive(runner("smx_chroma_cqt_f32_dev", lead * 12 * frames, np.float32, (12, kind, p)), CQT_PLACEMENTS,
          lambda res, pl: same(res, [bits], ("chroma_cqt is of_cqt of the magnitudes", pl)))
    folded = CR.of_cqt(r, mag.astype(np.float64), 12, "inf")
    drive(plane_call("smx_chroma_of_cqt_f32_dev", mag, [(lead, 12, frames)], (c._h,), (12, kind, p)), [(0, 0), (1, 1), (3, 1)],
          lambda res, pl: np.testing.assert_allclose(host(res[0], np.float32, folded.shape), folded, rtol=2e-6, atol=2e-6 * float(np.max(np.abs(folded)))))


# ---- row 14: the streaming entries -----------------------------------------------------------------------------------------

def streamed(step, flush, handle, x, cuts, rows_out, dtype, capacity, pending, pl):
    """three chunks, then the flush, every one into a guarded window; (x_off, x_stride - m, out_off, out_stride - capacity)"""
    import torch
    x_off, x_pad, o_off, o_pad = pl
    parts = []

    def emit(entry, cap, *head):
        count = C.c_int64()
        cap = max(1, int(cap))
        out = Region.out(rows_out, cap, dtype, o_off, o_pad)
        call(entry, handle, *head, out, cap + o_pad, C.byref(count))
        if count.value:
            parts.append(out.collect(count.value, tail_free=True))
    for a, b in zip(cuts[:-1], cuts[1:]):
        emit(step, capacity(b - a), Region.of(x[:, a:b], x_off, x_pad), b - a, b - a + x_pad)
    emit(flush, pending())
    return [torch.cat(parts, dim=1)]


@row("smx_stft_kernel_step_dev")
def test_stft_stream():
    """Stft.Kernel fed from rows m + 3 apart; its window's pitch is the capacity, so the output moves by an offset only.  The
    frames total Stft.transform of the whole signal (the oracle, at the north-star rule)"""
    fft, hop, channels, n = 256, 64, 2, 3000
    c, _ = configs(fft, hop)
    x = signal(14, channels, n)
    want = transform_oracle(fft, hop, 14, channels, n)
    bins, frames = want.shape[1:]
    width = fft + Stft.left_width(c) + Stft.right_width(c)

    def run(pl):
        k = Stft.Kernel.prepare(c, np.float32, channels, 1000)
        return streamed("smx_stft_kernel_step_dev", "smx_stft_kernel_flush_dev", k._h, x, [0, 1000, 2000, 3000], channels * bins, np.complex64,
                        lambda m: (m + width) // hop + 2, lambda: (fft + width) // hop + 2, pl)
    drive(run, [(0, 0, 0, 0), (1, 3, 1, 0), (0, 3, 0, 0)], lambda res, pl: fast_gate(host(res[0], np.complex64, want.shape), want, pl))


@row("smx_cqt_kernel_step_f32_dev")
def test_cqt_stream():
    """Cqt.Kernel with both strides padded: the columns total the offline transform bit for bit (test_gpu_cqt_stream's law)"""
    import torch
    c = Cqt.Config.create(n_bins=36, sample_rate=22050, fmin=16 * Cqt.C1, hop=63)
    channels, n = 2, 4096
    x = signal(15, channels, n)
    whole = Cqt.transform(c, torch.from_numpy(np.array(x)).cuda())
    bits = torch.view_as_real(whole.contiguous()).view(torch.int32).reshape(channels * c.n_bins, -1)

    def run(pl):
        k = Cqt.Kernel.prepare(c, channels=channels, max_block=n)
        return streamed("smx_cqt_kernel_step_f32_dev", "smx_cqt_kernel_flush_f32_dev", k._h, x, [0, 1500, 3000, n], channels * c.n_bins, np.complex64,
                        lambda m: lib.smx_cqt_kernel_columns_after(k._h, m), lambda: lib.smx_cqt_kernel_pending(k._h), pl)
    drive(run, [(0, 0, 0, 0), (1, 3, 1, 5), (0, 1, 0, 64)], lambda res, pl: same(res, [bits], ("offline transform", pl)))


@row("smx_resample_kernel_step_f32_dev", "smx_resample_stream_step_f32_dev")
def test_resample_streams():
    """the block-carry kernel of a x2 stage and the direct stream of 5 -> 7, y_stride padded: the chunks total the offline call
    bit for bit (the partition laws of test_gpu_resample_stream / test_gpu_resample_config), which rows 12 tie to the oracle"""
    import torch
    channels, n = 2, 9001
    x = signal(16, channels, n)
    xd = torch.from_numpy(np.array(x)).cuda()
    cuts = [0, 3000, 6000, n]
    placements = [(0, 0, 0, 0), (1, 3, 1, 3), (0, 1, 0, 64)]
    proto = Resample.prototype(2, 160, 0.45 / 2, O.kaiser_beta(100.0))
    st = Resample.Stage.create(proto, 2, 1, 160)
    whole = Resample.Stage.apply(st, xd).contiguous().view(torch.int32)

    def run_kernel(pl):
        k = Resample.Kernel.prepare(st, channels, 3001)
        return streamed("smx_resample_kernel_step_f32_dev", "smx_resample_kernel_flush_f32_dev", k._h, x, cuts, channels, np.float32,
                        lambda m: lib.smx_resample_kernel_out_bound(k._h, m), lambda: lib.smx_resample_kernel_pending(k._h), pl)
    drive(run_kernel, placements, lambda res, pl: same(res, [whole], ("Stage.apply", pl)))
    cfg = Resample.Config.create(5, 7)
    whole_cfg = Resample.apply(cfg, xd).contiguous().view(torch.int32)

    def run_stream(pl):
        k = Resample.Kernel.prepare(cfg, channels, 3001)
        return streamed("smx_resample_stream_step_f32_dev", "smx_resample_stream_flush_f32_dev", k._h, x, cuts, channels, np.float32,
                        lambda m: lib.smx_resample_stream_out_bound(k._h, m), lambda: lib.smx_resample_stream_pending(k._h), pl)
    drive(run_stream, placements, lambda res, pl: same(res, [whole_cfg], ("Resample.apply", pl)))


@row("smx_stft_synthesis_step_dev")
def test_synthesis_stream():
    """Stft.Synthesis: chunks of frames one complex element in, samples into an offset window; the stream totals Stft.invert,
    which test_invert_* tie to the oracle"""
    import torch
    fft, hop, channels, frames = 256, 64, 2, 30
    c, o = configs(fft, hop)
    bins = fft // 2 + 1
    z = random_spectrum(17, channels, bins, frames, np.complex64)
    whole = Stft.invert(c, torch.from_numpy(z).cuda()).contiguous().view(torch.int32)
    fast_gate(host(whole, np.float32)[None], O.invert(o, z, None)[None], "Stft.invert")

    def run(pl):
        s = Stft.Synthesis.prepare(c, np.complex64, channels, 10)
        parts = []

        def emit(entry, cap, *head):
            count = C.c_int64()
            out = Region.out(channels, cap, np.float32, pl[1])
            call(entry, s._h, *head, out, cap, C.byref(count))
            if count.value:
                parts.append(out.collect(count.value, tail_free=True))
        for a in (0, 10, 20):
            emit("smx_stft_synthesis_step_dev", max(10 * hop, fft) + hop, Region.of(z[:, :, a:a + 10], pl[0]), bins, 10)
        emit("smx_stft_synthesis_flush_dev", fft + hop)
        return [torch.cat(parts, dim=1)]
    drive(run, [(0, 0), (1, 1), (1, 2)], lambda res, pl: same(res, [whole], ("Stft.invert", pl)))


# ---- the Python face -------------------------------------------------------------------------------------------------------

def test_python_face_on_offset_views():
    """_tensor.Batch keeps x.contiguous(): a contiguous view with a storage offset arrives 4 bytes off (a complex one 8)"""
    import torch

    def view_of(a):
        a = np.ascontiguousarray(a)
        t = torch.tensor(a, device="cuda")
        buf = torch.empty(a.size + 2, dtype=t.dtype, device="cuda")
        v = buf[1:1 + a.size].view(a.shape)
        v.copy_(t)
        assert v.is_contiguous() and v.data_ptr() % (2 * t.element_size()) == t.element_size()
        return v

    def bits(t):
        t = torch.view_as_real(t) if t.is_complex() else t
        return t.contiguous().view(torch.int32)
    c, _ = configs(2048, 512)
    lead, n = 3, 512 * 47
    x = signal(18, lead, n)
    z = random_spectrum(19, 2, 1025, 40, np.complex64)
    plan = Fir.Plan.create(Fir.design_lowpass(600, 0.25, 80.0))
    st = Resample.Stage.create(Resample.prototype(2, 160, 0.45 / 2, O.kaiser_beta(100.0)), 2, 1, 160)
    power = np.abs(x) + np.float32(1e-3)
    faces = [("power_spectrum", lambda t: Stft.power_spectrum(c, t), x), ("transform", lambda t: Stft.transform(c, t), x),
             ("Fir.apply", lambda t: Fir.apply(plan, t), x), ("Stage.apply", lambda t: Resample.Stage.apply(st, t), x),
             ("invert", lambda t: Stft.invert(c, t), z), ("power_to_db", lambda t: S.power_to_db(t, top_db=80.0), power),
             ("amplitude_to_db", lambda t: S.amplitude_to_db(t, top_db=80.0), x)]
    for name, face, a in faces:
        v = view_of(a)
        if not v.is_complex():
            assert v.data_ptr() % 8 == 4
        assert torch.equal(bits(face(v)), bits(face(v.clone()))), name


# ---- the coverage law ------------------------------------------------------------------------------------------------------

def test_coverage_law():
    """every `*_dev` entry point of the header runs in a row above, or is excluded by name with a reason (no GPU work)"""
    with open(os.path.join(ROOT, "include", "soundml_amd.h")) as fh:
        declared = set(re.findall(r"\b(smx_\w+_dev)\s*\(", fh.read()))
    assert len(declared) > 40
    for name in EXCLUDED:
        assert name in declared and (name.startswith("smx_debug_") or "_flush_" in name or name == "smx_resample_shape_c128_dev"), name
    missing = sorted(declared - set(TABLE) - set(EXCLUDED))
    assert not missing, "device entry points without a placement row: %s" % ", ".join(missing)
    assert not sorted((set(TABLE) | set(EXCLUDED)) - declared)
