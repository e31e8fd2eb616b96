"""Streams: every device entry point on a held side stream.

The other GPU tests run on the null stream, where a launch, memset, copy or scratch allocation that lost the caller's stream is
invisible (every job struct's stream defaults to the null one).  Here each public Python face runs under a FENCE on a
`torch.cuda.Stream()`, which does not block against the null stream:

  1. the inputs are prepared and the expected bits computed by the ordinary call on the default stream (those bits are pinned to
     the oracle or a restatement by the other files; this one compares bit for bit, NaN equal to NaN);
  2. on the side stream: fresh input tensors are filled with a DECOY (the source reversed and halved: finite, non-negative where
     the source is), the stream is drained, then HELD for H milliseconds, and the true inputs are copied over the decoy behind
     the hold; the face is called and `pending = not side.query()` is read at once;
  3. after `side.synchronize()` the outputs must equal the expected bits.

Work that the call put on any other stream runs during the hold: it reads the decoy, or scratch not yet produced, and the bits
differ (test_a_wrong_stream_launch_reads_the_decoy shows that the harness sees exactly this).  A call that comes back with the
stream still held did not synchronise: that is the law for every row but those that declare `synchronises`, which must come back
with the stream idle.  They are the faces documented to read a flag back: the four spectral-shape features (include/soundml_amd.h:
"That last check reads the data, so the _dev entry points synchronise the stream before returning") and
spectral_contrast_of_spectrogram ("The flat spectrogram face reads back one flag ... as the spectral-shape features do;
nothing else synchronises the caller's stream").  `pending` alone misses a call that waits for the device in its middle and
launches more afterwards, so a warm call must also be back within H / 2: what takes longer builds tables per call or waits.
While a row runs, every function of the library whose declaration ends in `void *stream)` is wrapped: the handles it received must
all be the side stream's, and the names it saw must be the row's declared entries.  test_coverage_law holds the table against the
header.

The hold.  `torch.cuda._sleep`, calibrated once per session with a pair of events (a chain of matmuls if it proves unusable): on an
MI355X 2.39e6 cycles per millisecond, a 50 ms hold measured 49.9 ms.  H_MS comes from host_return_times() on that machine: the
largest warm host-side return of any row on the default stream is 0.68 ms (stft_kernel-256-64: three steps and the flush; every
single-call row is under 0.4 ms), ten times that is 6.8 ms, so H_MS is the floor of 50.  The whole file (403 tests) runs in 24 s.

What the file found when it was written (each fails on the library as it was): the runtime's hipFreeAsync blocks the host when it
frees a block that the stream-ordered pool handed out again on the stream of its previous, not yet executed, free -- so the second
call in a row on a busy stream waited for the device (test_two_calls_in_a_row_stay_pending), as did one call that takes two scratch
arrays of a size in turn: Griffin-Lim, hpss and Stft.Synthesis on the generic ISTFT, every Stft.Kernel step (99 ms of a 100 ms
hold each); pitch_shift built and freed a resampler per call (hipFree waits for the device); and the synchronising faces queued
their scratch release behind the wait, so the stream was not idle when they returned.
"""
import contextlib
import ctypes as C
import os
import re
import time

import numpy as np
import pytest

import soundml_amd as S
from soundml_amd import Chroma, Convert, Cqt, Decompose, Effects, Fir, Mel, Resample, Sequence, Stft
from soundml_amd import energy as Energy
from soundml_amd import onset as Onset
from soundml_amd._lib import check, lib
from conftest import ROOT
from oracle import soundml_oracle as O

pytestmark = pytest.mark.gpu

H_MS = 50.0             # see the docstring: ten times the largest warm host-side return, at least 50
FAST_OFF = {"SMX_DISABLE_FAST": "1"}
SR = 22050

TABLE = {}              # entry point -> the rows that run it
ROWS = []
EXCLUDED = {
    "smx_debug_stft_transform_frame_major_f32_dev": "diagnostic face",
    "smx_debug_cqt_project_f32_dev": "diagnostic face",
    "smx_synchronize": "test_synchronize_drains_its_stream_alone",
}


def header_stream_entries():
    with open(os.path.join(ROOT, "include", "soundml_amd.h")) as fh:
        text = fh.read()
    names = re.findall(r"\b(smx_\w+)\s*\([^;{}]*?void\s*\*\s*stream\s*\)\s*;", text)
    assert len(names) == len(set(names)) == len(re.findall(r"void\s*\*\s*stream\s*\)", text)), "the header's stream entries did not parse one to one"
    return sorted(names)


STREAM_ENTRIES = header_stream_entries()


class Case:
    """inputs: host arrays; call(cfg, state, *device tensors) -> tensor(s); make(cold) -> a fresh configuration (cold: one whose
    lazily built tables nothing else in the process has built); state(cfg) -> a fresh streaming object or None"""

    def __init__(self, inputs, call, make=None, state=None, env=None):
        self.inputs = [np.ascontiguousarray(a) for a in inputs]
        self.call, self.env = call, env
        self.make = make or (lambda cold: None)
        self.state = state or (lambda cfg: None)


class Row:
    def __init__(self, fn, param, entries, synchronises, cold):
        self.fn, self.param, self.entries, self.synchronises, self.cold = fn, param, frozenset(entries), synchronises, cold
        parts = param if isinstance(param, tuple) else (param,)
        self.id = fn.__name__ if param is None else "%s-%s" % (fn.__name__, "-".join(getattr(p, "__name__", str(p)).replace(" ", "") for p in parts))

    def case(self):
        return self.fn() if self.param is None else self.fn(self.param)


def width(entry, param):
    """"smx_mel_apply_{f}_dev" -> ..._f32_dev or ..._f64_dev, "{c}" -> c64 or c128, by the dtype among the row's parameters"""
    if "{" not in entry:
        return entry
    dtype = [p for p in (param if isinstance(param, tuple) else (param,)) if isinstance(p, type)][0]
    narrow = dtype in (np.float32, np.complex64)
    return entry.format(f="f32" if narrow else "f64", c="c64" if narrow else "c128")


def row(*entries, params=(None,), synchronises=False, cold=False):
    """entries: the stream-taking entry points the row runs, all of them (the recorder holds the row to this)"""
    def mark(fn):
        for p in params:
            ran = [width(e, p) for e in entries]
            for e in ran:
                TABLE.setdefault(e, []).append(fn.__name__)
            ROWS.append(Row(fn, p, ran, synchronises, cold))
        return fn
    return mark


@pytest.fixture(autouse=True)
def _default_interior():
    S.set_interior("float32")
    yield
    S.set_interior("float32")


@contextlib.contextmanager
def environment(env):
    """the overrides the library reads per call, put back afterwards"""
    env = dict(env or {})
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


# ---- the hold, the recorder, the fence -------------------------------------------------------------------------------------

def elapsed_ms(work):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    work()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


class Hold:
    """hold(ms) keeps the current stream busy for about that long"""

    def __init__(self):
        import torch
        torch.cuda._sleep(1000)
        torch.cuda.synchronize()
        cycles = 20_000_000
        ms = elapsed_ms(lambda: torch.cuda._sleep(cycles))
        self.kind, self.per_ms = "sleep", cycles / max(ms, 1e-6)
        if not 0.5 * H_MS <= elapsed_ms(lambda: self(H_MS)) <= 4 * H_MS:     # _sleep is not usable here: a fixed chain of matmuls
            self.kind = "matmul"
            self.a = torch.randn(2048, 2048, device="cuda")
            self.b = torch.empty_like(self.a)
            torch.mm(self.a, self.a, out=self.b)
            torch.cuda.synchronize()
            self.per_ms = 64 / elapsed_ms(lambda: [torch.mm(self.a, self.a, out=self.b) for _ in range(64)])
        self.measured = elapsed_ms(lambda: self(H_MS))
        assert 0.5 * H_MS <= self.measured <= 4 * H_MS, "a hold of %g ms took %g ms (%s)" % (H_MS, self.measured, self.kind)

    def __call__(self, ms):
        import torch
        count = max(1, int(ms * self.per_ms))
        if self.kind == "sleep":
            torch.cuda._sleep(count)
        else:
            for _ in range(count):
                torch.mm(self.a, self.a, out=self.b)


@pytest.fixture(scope="module")
def hold():
    """the calibrated hold, once the control has shown that a trivial launch behind it comes back pending"""
    import torch
    h = Hold()
    side = torch.cuda.Stream()
    assert side.cuda_stream != 0
    with torch.cuda.stream(side):
        x = torch.zeros(16, device="cuda")
        side.synchronize()
        h(H_MS)
        x.add_(0)
        pending = not side.query()
    side.synchronize()
    assert pending, "the hold is broken: a trivial launch behind %g ms of %s was not pending" % (H_MS, h.kind)
    return h


@contextlib.contextmanager
def recording():
    """every (name, stream handle) a stream-taking entry point of the library receives; a call without a stream and without an
    output is the faces' parameter check (no clips, no device work) and is left out"""
    log, saved = [], {}

    def wrap(name, fn):
        def wrapper(*args):
            st = args[-1]
            handle = st.value if isinstance(st, C.c_void_p) else st
            if not (handle is None and len(args) > 1 and args[-2] is None):
                log.append((name, int(handle or 0)))
            return fn(*args)
        return wrapper
    try:
        for name in STREAM_ENTRIES:
            saved[name] = getattr(lib, name)
            setattr(lib, name, wrap(name, saved[name]))
        yield log
    finally:
        for name, fn in saved.items():
            setattr(lib, name, fn)


def decoy(a):
    """the source reversed and halved: finite, the same shape and sign, clearly different"""
    return np.ascontiguousarray(a[..., ::-1] * a.dtype.type(0.5))


def other(a):
    """different data of the same kind for the second stream"""
    return np.ascontiguousarray(np.roll(a, 7, axis=-1)[..., ::-1] * a.dtype.type(0.75))


def device(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def flat(out):
    if out is None:
        return []
    if isinstance(out, (tuple, list)):
        return [t for o in out for t in flat(o)]
    return [out]


def bits(t):
    import torch
    t = torch.view_as_real(t.contiguous()) if t.is_complex() else t.contiguous()
    return t.reshape(-1).view(torch.int32)


def same_bits(got, want, what):
    import torch
    assert len(got) == len(want), (what, len(got), len(want))
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and g.dtype == w.dtype, (what, k, g.shape, w.shape)
        if not torch.equal(bits(g), bits(w)):
            d = (bits(g) != bits(w)).nonzero()
            raise AssertionError("%s: result %d differs from the default stream's in %d words of %d, the first at %d" % (
                what, k, d.shape[0], bits(g).numel(), int(d[0])))


def ordinary(case, cfg, arrays):
    """the ordinary call: the default stream, fresh tensors, a fresh state"""
    import torch
    xs = [device(a) for a in arrays]
    with environment(case.env):
        out = flat(case.call(cfg, case.state(cfg), *xs))
    torch.cuda.synchronize()
    return out


class Placed:
    """one stream's side of the fence: decoys in fresh tensors, then (release) the hold and the true inputs behind it"""

    def __init__(self, side, arrays):
        import torch
        self.side = side
        self.true = [device(a) for a in arrays]
        fake = [device(decoy(a)) for a in arrays]
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            self.xs = [torch.empty_like(t) for t in self.true]
            for x, d in zip(self.xs, fake):
                x.copy_(d)
        side.synchronize()                  # a stray launch finds the decoy, not what the allocator left there

    def hold(self, hold, ms):
        import torch
        with torch.cuda.stream(self.side):
            hold(ms)
            for x, t in zip(self.xs, self.true):
                x.copy_(t, non_blocking=True)

    def run(self, case, cfg, state):
        """-> (outputs, pending, seconds the call took to return)"""
        import torch
        with torch.cuda.stream(self.side), environment(case.env):
            t0 = time.perf_counter()
            out = case.call(cfg, state, *self.xs)
            pending = not self.side.query()
            dt = time.perf_counter() - t0
        return flat(out), pending, dt


def fenced(hold, case, cfg, state, arrays, entries):
    """one pass of the fence -> (outputs, pending, seconds): the handles and the names are checked here"""
    import torch
    side = torch.cuda.Stream()
    assert side.cuda_stream != 0
    p = Placed(side, arrays)
    p.hold(hold, H_MS)
    with recording() as log:
        out, pending, dt = p.run(case, cfg, state)
    side.synchronize()
    wrong = sorted({(n, h) for n, h in log if h != side.cuda_stream})
    assert not wrong, "entry points that were not given the caller's stream %#x: %s" % (side.cuda_stream, wrong)
    assert {n for n, _ in log} == set(entries), "the row declares %s and ran %s" % (sorted(entries), sorted({n for n, _ in log}))
    return out, pending, dt


# ---- helpers for the rows --------------------------------------------------------------------------------------------------

def sig(seed, *shape, dtype=np.float32):
    return np.random.default_rng(seed).uniform(-1, 1, size=shape).astype(dtype)


def mags(seed, *shape, dtype=np.float32):
    return (np.abs(np.random.default_rng(seed).standard_normal(shape)) + 0.01).astype(dtype)


def spectrum(seed, *shape, dtype=np.complex64):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(dtype)


def stft_config(fft, hop, cold=False, **kw):
    return Stft.Config.create(fft_size=fft, hop=hop, window="hamming" if cold else "hann", **kw)


def mel_config(n_mels, sr, fft, cold=False):
    return Mel.Config.create(n_mels=n_mels, sample_rate=sr, fft_size=fft, f_min=20.0 if cold else 0.0)


def chunks(x, cuts):
    return [x[..., a:b] for a, b in zip(cuts[:-1], cuts[1:])]


def streamed(k, x, cuts, flush=None):
    """three unequal chunks and the flush through a streaming object -> the concatenated output"""
    import torch
    parts = flat([k.step(c) for c in chunks(x, cuts)]) + flat(flush(k) if flush else k.flush())
    return torch.cat(parts, dim=-1)


# ---- rows: analysis --------------------------------------------------------------------------------------------------------

@row("smx_stft_power_range_f32_dev", cold=True,
     params=[(2048, 512, "fast"), (2048, 512, "general"), (1024, 256, "fast"), (256, 64, "fast"), (4096, 1024, "fast"), (100, 33, "fast")])
def power_spectrum(p):
    fft, hop, route = p
    return Case([sig(1, 2, hop * 39 + 17)], lambda c, s, x: Stft.power_spectrum(c, x, power=1.0), lambda cold: stft_config(fft, hop, cold),
                env=FAST_OFF if route == "general" else None)


@row("smx_stft_transform_range_f32_dev", cold=True, params=[(2048, 512), (1024, 256), (100, 33)])
def transform(p):
    return Case([sig(2, 2, p[1] * 39 + 17)], lambda c, s, x: Stft.transform(c, x), lambda cold: stft_config(*p, cold))


@row("smx_stft_transform_range_f64_dev", cold=True)
def transform_float64():
    return Case([sig(3, 2, 9 * 512 + 123, dtype=np.float64)], lambda c, s, x: Stft.transform(c, x), lambda cold: stft_config(512, 128, cold))


@row("smx_stft_power_range_f64_dev", cold=True)
def power_float64():
    return Case([sig(4, 2, 9 * 512 + 123, dtype=np.float64)], lambda c, s, x: Stft.power_range(c, x, 1, 30), lambda cold: stft_config(512, 128, cold))


@row("smx_mel_spectrogram_f32_dev", cold=True, params=[(2048, 512, "fast"), (2048, 512, "general"), (1024, 256, "fast"), (512, 128, "fast")])
def mel_spectrogram(p):
    fft, hop, route = p
    return Case([sig(5, 2, hop * 39)], lambda c, s, x: S.mel_spectrogram(c[0], c[1], x), lambda cold: (stft_config(fft, hop, cold), mel_config(40, SR, fft, cold)),
                env=FAST_OFF if route == "general" else None)


@row("smx_mfcc_f32_dev", cold=True, params=[(2048, 512), (1024, 256)])
def mfcc(p):
    fft, hop = p
    return Case([sig(6, 2, hop * 39)], lambda c, s, x: S.mfcc(c[0], c[1], x, n_mfcc=13, lifter=22.0),
                lambda cold: (stft_config(fft, hop, cold), mel_config(40, SR, fft, cold)))


@row("smx_chroma_stft_f32_dev", cold=True, params=[(2048, 512), (1024, 256)])
def chroma_stft(p):
    fft, hop = p
    return Case([sig(7, 2, hop * 39)], lambda c, s, x: S.chroma_stft(c[0], c[1], x),
                lambda cold: (stft_config(fft, hop, cold), Chroma.Config.create(SR, fft, tuning=0.25 if cold else 0.0)))


@row("smx_mel_apply_{f}_dev", cold=True, params=[np.float32, np.float64])
def mel_apply(dtype):
    return Case([mags(8, 2, 257, 37, dtype=dtype)], lambda c, s, x: Mel.apply(c, x), lambda cold: mel_config(40, SR, 512, cold))


@row("smx_chroma_apply_f32_dev", cold=True)
def chroma_apply():
    return Case([mags(9, 2, 257, 37)], lambda c, s, x: Chroma.apply(c, x, norm="inf"), lambda cold: Chroma.Config.create(SR, 512, tuning=0.25 if cold else 0.0))


# ---- rows: decibels and the way back ---------------------------------------------------------------------------------------

@row("smx_power_to_db_f32_dev", params=[80.0, "unclamped"])
def power_to_db(top_db):
    top_db = None if top_db == "unclamped" else top_db
    return Case([mags(10, 3, 4099)], lambda c, s, x: S.power_to_db(x, reference=2.0, top_db=top_db))


@row("smx_amplitude_to_db_f32_dev", params=[80.0, "unclamped"])
def amplitude_to_db(top_db):
    top_db = None if top_db == "unclamped" else top_db
    return Case([sig(11, 3, 4099)], lambda c, s, x: S.amplitude_to_db(x, reference=2.0, top_db=top_db))


@row("smx_db_to_power_{f}_dev", params=[np.float32, np.float64])
def db_to_power(dtype):
    return Case([sig(12, 1000, dtype=dtype) * dtype(40)], lambda c, s, x: Convert.db_to_power(x, reference=0.5))


@row("smx_db_to_amplitude_{f}_dev", params=[np.float32, np.float64])
def db_to_amplitude(dtype):
    return Case([sig(13, 1000, dtype=dtype) * dtype(40)], lambda c, s, x: Convert.db_to_amplitude(x, reference=0.5))


@row("smx_mel_invert_{f}_dev", cold=True,
     params=[(np.float32, "wave"), (np.float32, "general"), (np.float64, "wave"), (np.float64, "general")])
def mel_invert(p):
    dtype, route = p
    return Case([mags(14, 2, 80, 19, dtype=dtype)], lambda c, s, m: Mel.invert(c, m, n_iter=7), lambda cold: mel_config(80, 16000, 400, cold),
                env=FAST_OFF if route == "general" else None)


@row("smx_mel_invert_f32_dev", cold=True)
def mel_to_stft():
    return Case([mags(15, 2, 8, 37)], lambda c, s, m: S.mel_to_stft(c, m, power=2.0, n_iter=7), lambda cold: mel_config(8, 8000, 64, cold))


@row("smx_mfcc_to_mel_{f}_dev", params=[np.float32, np.float64])
def mfcc_to_mel(dtype):
    return Case([sig(16, 2, 13, 70, dtype=dtype) * dtype(10)], lambda c, s, m: S.mfcc_to_mel(m, 40, 22.0, 0.5))


@row("smx_mel_invert_f32_dev", "smx_stft_griffin_lim_f32_dev", cold=True, params=[(2048, 512), (512, 128)])
def mel_to_audio(p):
    fft, hop = p
    return Case([mags(17, 2, 40, 20)], lambda c, s, m: S.mel_to_audio(c[0], c[1], m, n_iter=5, gl_iter=2),
                lambda cold: (stft_config(fft, hop, cold), mel_config(40, SR, fft, cold)))


@row("smx_mfcc_to_mel_f32_dev", "smx_mel_invert_f32_dev", "smx_stft_griffin_lim_f32_dev", cold=True)
def mfcc_to_audio():
    return Case([sig(18, 2, 13, 20) * np.float32(10)], lambda c, s, m: S.mfcc_to_audio(c[0], c[1], m, lifter=22.0, n_iter=5, gl_iter=2),
                lambda cold: (stft_config(2048, 512, cold), mel_config(40, SR, 2048, cold)))


# ---- rows: synthesis -------------------------------------------------------------------------------------------------------

@row("smx_stft_griffin_lim_f32_dev", cold=True, params=[(2048, 512, False), (2048, 512, True), (1024, 256, False), (100, 25, False)])
def griffin_lim(p):
    fft, hop, phase = p
    s = mags(19, 2, fft // 2 + 1, 20)
    if phase:
        return Case([s, sig(20, *s.shape) * np.float32(3)], lambda c, st, m, ph: Stft.griffin_lim(c, m, n_iter=3, init=ph, length=hop * 19 - 5),
                    lambda cold: stft_config(fft, hop, cold))
    return Case([s], lambda c, st, m: Stft.griffin_lim(c, m, n_iter=3), lambda cold: stft_config(fft, hop, cold))


@row("smx_stft_invert_f32_dev", cold=True,
     params=[(2048, 512, None, "pipeline"), (2048, 512, 512 * 23 - 1, "pipeline"), (2048, 512, None, "tiles"), (2048, 512, None, "general"),
             (1024, 256, None, "pipeline"), (100, 25, 501, "pipeline")])
def invert(p):
    fft, hop, length, route = p
    env = {"pipeline": None, "tiles": {"SMX_INVERT_PIPELINE": "0"}, "general": FAST_OFF}[route]
    return Case([spectrum(21, 2, fft // 2 + 1, 24)], lambda c, s, z: Stft.invert(c, z, length=length), lambda cold: stft_config(fft, hop, cold), env=env)


@row("smx_stft_invert_f64_dev", cold=True)
def invert_float64():
    return Case([spectrum(22, 2, 257, 23, dtype=np.complex128)], lambda c, s, z: Stft.invert(c, z), lambda cold: stft_config(512, 128, cold))


# ---- rows: the spectrogram-domain features ---------------------------------------------------------------------------------

PLANE = (2, 257, 37)


@row("smx_spectral_centroid_f32_dev", synchronises=True)
def spectral_centroid():
    return Case([mags(23, *PLANE)], lambda c, s, x: S.spectral_centroid(x, sample_rate=SR))


@row("smx_spectral_bandwidth_f32_dev", synchronises=True, params=["own", "given"])
def spectral_bandwidth(centroid):
    if centroid == "own":
        return Case([mags(24, *PLANE)], lambda c, s, x: S.spectral_bandwidth(x, sample_rate=SR))
    return Case([mags(24, *PLANE), mags(25, 2, 1, 37) * np.float32(3000)], lambda c, s, x, ce: S.spectral_bandwidth(x, sample_rate=SR, centroid=ce))


@row("smx_spectral_rolloff_f32_dev", synchronises=True)
def spectral_rolloff():
    return Case([mags(26, *PLANE)], lambda c, s, x: S.spectral_rolloff(x, sample_rate=SR))


@row("smx_spectral_flatness_f32_dev", synchronises=True)
def spectral_flatness():
    return Case([mags(27, *PLANE)], lambda c, s, x: S.spectral_flatness(x))


@row("smx_spectral_contrast_dev_f32", cold=True, params=[(2048, 512), (512, 128)])
def spectral_contrast(p):
    return Case([sig(28, 2, p[1] * 39)], lambda c, s, x: S.spectral_contrast(c, x, sample_rate=SR), lambda cold: stft_config(*p, cold))


@row("smx_spectral_contrast_of_spectrogram_dev_f32", synchronises=True)     # "the flat spectrogram face reads back one flag"
def spectral_contrast_of_spectrogram():
    return Case([mags(29, *PLANE)], lambda c, s, x: S.spectral_contrast_of_spectrogram(x, sample_rate=SR))


@row("smx_onset_strength_dev_f32", cold=True, params=[(2048, 512), (512, 128)])
def onset_strength(p):
    fft, hop = p
    return Case([sig(30, 2, hop * 39)], lambda c, s, x: S.onset_strength(c[0], c[1], x, lag=2),
                lambda cold: (stft_config(fft, hop, cold), mel_config(40, SR, fft, cold)))


@row("smx_onset_flux_dev_f32")
def onset_flux():
    return Case([sig(31, 2, 40, 37) * np.float32(40)], lambda c, s, x: Onset.flux(x, lag=2))


@row("smx_hpss_masks_f32_dev", params=[(31, 31, "fast"), (31, 31, "general"), (17, 31, "fast"), (5, 9, "fast")])
def hpss_masks(p):
    return Case([mags(32, *PLANE)], lambda c, s, x: S.hpss_masks(x, kernel_size=p[:2], power=2.0, margin=(1.0, 2.0)), env=FAST_OFF if p[2] == "general" else None)


@row("smx_hpss_of_spectrogram_f32_dev", params=[(31, 31), (17, 31)])
def hpss_of_spectrogram(kernel):
    return Case([mags(33, *PLANE)], lambda c, s, x: S.hpss_of_spectrogram(x, kernel_size=kernel))


@row("smx_hpss_of_stft_c64_dev", params=[(31, 31), (17, 31)])
def hpss_of_stft(kernel):
    return Case([spectrum(34, *PLANE)], lambda c, s, z: S.hpss_of_stft(z, kernel_size=kernel))


@row("smx_hpss_f32_dev", cold=True, params=[(2048, 512, (31, 31)), (2048, 512, (17, 31)), (256, 64, (31, 31))])
def hpss(p):
    fft, hop, kernel = p
    return Case([sig(35, 2, 6000)], lambda c, s, x: S.hpss(c, x, kernel_size=kernel, margin=(1.0, 2.0)), lambda cold: stft_config(fft, hop, cold))


# ---- rows: effects ---------------------------------------------------------------------------------------------------------

def vocoder_config(cold):
    return stft_config(256, 64, cold, pad=("constant", 0.0))


@row("smx_phase_vocoder_{c}_dev", params=[(np.complex64, "independent"), (np.complex64, "locked"), (np.complex128, "locked")])
def phase_vocoder(p):
    return Case([spectrum(36, 3, 129, 30, dtype=p[0])], lambda c, s, z: Effects.phase_vocoder(c, z, 1.37, phase=p[1]), vocoder_config)


@row("smx_time_stretch_f32_dev", cold=True, params=[0.75, 1.6])
def time_stretch(rate):
    return Case([sig(37, 2, 4000)], lambda c, s, x: Effects.time_stretch(c, x, rate), vocoder_config)


@row("smx_pitch_shift_f32_dev", cold=True, params=[(3, 2), (4, 5)])
def pitch_shift(ratio):
    return Case([sig(38, 2, 4000)], lambda c, s, x: Effects.pitch_shift(c, x, ratio), vocoder_config)


# ---- rows: FIR, the resampler, constant-Q ----------------------------------------------------------------------------------

@row("smx_fir_apply_f32_dev", cold=True, params=[63, 80, 81, 200, 600])
def fir(taps):
    """fir_direct_kernel up to 80 taps, the FFT blocks from 81 on (fir.hip: the measured crossover), at two block sizes"""
    return Case([sig(taps, 2, 5001)], lambda c, s, x: Fir.apply(c, x), lambda cold: Fir.Plan.create(Fir.design_lowpass(taps, 0.2 if cold else 0.25, 80.0)))


def stage_x2(cold=False):
    return Resample.Stage.create(Resample.prototype(2, 160, (0.40 if cold else 0.45) / 2, O.kaiser_beta(100.0)), 2, 1, 160)


@row("smx_resample_stage_apply_f32_dev", cold=True, params=[(2, 1, 160), (1, 2, 161), (3, 2, 60)])
def resample_stage(p):
    l, m, k = p
    return Case([sig(39, 2, 6001)], lambda c, s, x: Resample.Stage.apply(c, x),
                lambda cold: Resample.Stage.create(Resample.prototype(l, k, (0.40 if cold else 0.45) / max(l, m), O.kaiser_beta(100.0)), l, m, k))


def resample_config(rate, cold, executor):
    c = Resample.Config.create(*rate, quality="best" if cold else "high")
    assert c.executor == executor
    return c


@row("smx_resample_stage_apply_f32_dev", cold=True)
def resample_apply_staged():
    return Case([sig(40, 2, 6001)], lambda c, s, x: Resample.apply(c, x), lambda cold: resample_config((24000, 48000), cold, "ols"))


@row("smx_resample_apply_f32_dev", cold=True)
def resample_apply_direct():
    return Case([sig(41, 2, 5001)], lambda c, s, x: Resample.apply(c, x), lambda cold: resample_config((5, 7), cold, "direct"))


@row("smx_resample_shape_c128_dev")
def resample_shape():
    """no Python face takes device memory here: the entry itself, as test_gpu_host_faces.shape_on_device calls it"""
    import torch
    n, k, lines = 2048, 5, 9
    h = O.ols_plan_spectrum(np.random.default_rng(42).uniform(-1, 1, size=2 * k + 1), n, 1, 1)

    def call(c, s, x, oh):
        out = torch.empty_like(x)
        check(lib.smx_resample_shape_c128_dev(C.c_void_p(x.data_ptr()), C.c_void_p(oh.data_ptr()), C.c_void_p(out.data_ptr()), lines, n, 1, 1,
                                              C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        return out
    return Case([spectrum(43, lines, n // 2 + 1, dtype=np.complex128), h.astype(np.complex128)], call)


def cqt_config(n_bins, cold=False):
    if n_bins == 36:        # three octaves: the halving resampler runs twice
        return Cqt.Config.create(n_bins=36, sample_rate=SR, fmin=16 * Cqt.C1, hop=63, tuning=0.25 if cold else 0.0)
    return Cqt.Config.create(n_bins=n_bins, sample_rate=SR, tuning=0.25 if cold else 0.0)      # one octave behind six early decimations


CQT = [(36, 4096), (7, 8192)]


@row("smx_cqt_transform_f32_dev", cold=True, params=CQT)
def cqt_transform(p):
    return Case([sig(44, 2, p[1])], lambda c, s, x: Cqt.transform(c, x), lambda cold: cqt_config(p[0], cold))


@row("smx_cqt_power_spectrum_f32_dev", cold=True, params=CQT)
def cqt_power_spectrum(p):
    return Case([sig(45, 2, p[1])], lambda c, s, x: Cqt.power_spectrum(c, x, power=1.0), lambda cold: cqt_config(p[0], cold))


@row("smx_chroma_cqt_f32_dev", cold=True, params=CQT)
def chroma_cqt(p):
    return Case([sig(46, 2, p[1])], lambda c, s, x: S.chroma_cqt(c, x), lambda cold: cqt_config(p[0], cold))


@row("smx_chroma_of_cqt_f32_dev", cold=True)
def chroma_of_cqt():
    return Case([mags(47, 2, 36, 41)], lambda c, s, x: Chroma.of_cqt(c, x, n_chroma=12, norm="inf"), lambda cold: cqt_config(36, cold))


# ---- rows: energy, pitch, rhythm, sequence, decompose ----------------------------------------------------------------------

FRAMES = [(2048, 512, 5000, "tile"), (2048, 512, 5000, "general"), (200, 64, 900, "tile"), (8, 11, 60, "tile")]


@row("smx_rms_device_f32", params=FRAMES)
def rms(p):
    fl, hop, n, route = p
    return Case([sig(48, 2, n)], lambda c, s, x: S.rms(x, frame_length=fl, hop=hop), env=FAST_OFF if route == "general" else None)


@row("smx_zero_crossing_rate_device_f32", params=FRAMES)
def zero_crossing_rate(p):
    fl, hop, n, route = p
    return Case([sig(49, 2, n)], lambda c, s, x: S.zero_crossing_rate(x, frame_length=fl, hop=hop), env=FAST_OFF if route == "general" else None)


@row("smx_rms_of_spectrogram_device_f32")
def rms_of_spectrogram():
    return Case([mags(50, 2, 129, 37)], lambda c, s, x: S.rms_of_spectrogram(x, frame_length=256))


PITCH = [(2048, 512, 5000, SR, 65.0, 2093.0, "tile"), (2048, 512, 5000, SR, 65.0, 2093.0, "general"), (200, 64, 900, 8000, 100.0, 1000.0, "tile")]


@row("smx_yin_resident_f32", params=PITCH)
def yin(p):
    fl, hop, n, sr, fmin, fmax, route = p
    return Case([sig(51, 2, n)], lambda c, s, x: S.yin(x, fmin, fmax, sample_rate=sr, frame_length=fl, hop=hop, return_aperiodicity=True),
                env=FAST_OFF if route == "general" else None)


@row("smx_yin_difference_resident_f32", params=PITCH)
def yin_difference(p):
    fl, hop, n, sr, fmin, fmax, route = p
    return Case([sig(52, 2, n)], lambda c, s, x: S.yin_difference(x, fmin, fmax, sample_rate=sr, frame_length=fl, hop=hop),
                env=FAST_OFF if route == "general" else None)


def pyin_tables(cold):
    return dict(n_thresholds=90 if cold else 100)          # the tables are cached by their parameters: another count, other tables


PYIN = [(256, 64, 1500, 8000, 400.0, 500.0), (2048, 512, 5000, SR, 65.0, 2093.0)]


@row("smx_pyin_accel_f32", cold=True, params=PYIN)
def pyin(p):
    fl, hop, n, sr, fmin, fmax = p
    return Case([sig(53, 2, n)], lambda c, s, x: S.pyin(x, fmin, fmax, sample_rate=sr, frame_length=fl, hop=hop, **c), pyin_tables)


@row("smx_pyin_observation_accel_f32", cold=True, params=PYIN)
def pyin_observation(p):
    fl, hop, n, sr, fmin, fmax = p
    return Case([sig(54, 2, n)], lambda c, s, x: S.pyin_observation(x, fmin, fmax, sample_rate=sr, frame_length=fl, hop=hop, **c), pyin_tables)


@row("smx_pyin_decode_accel_f32", params=[(61, 10, 40), (17, 70, 9)])
def pyin_decode(p):
    nb, h, count = p
    return Case([mags(55, 2, 2 * nb, count) * np.float32(0.1)], lambda c, s, x: S.pyin_decode(x, h))


def rhythm_tables(cold):
    return dict(win_length=48 if cold else 64)             # the window and the prior are cached by their parameters


@row("smx_rhythm_tempogram_gpu_f32", cold=True, params=["tile", "general"])
def tempogram(route):
    return Case([mags(56, 3, 200)], lambda c, s, x: S.tempogram(x, **c), rhythm_tables, env=FAST_OFF if route == "general" else None)


@row("smx_rhythm_tempo_gpu_f32", cold=True)
def tempo():
    return Case([mags(57, 3, 200)], lambda c, s, x: S.tempo(x, sample_rate=SR, hop=512, **c), rhythm_tables)


@row("smx_rhythm_beat_track_gpu_f32", cold=True, params=["tempo", 120.0])
def beat_track(bpm):
    bpm = None if bpm == "tempo" else bpm
    return Case([mags(58, 3, 200)], lambda c, s, x: S.beat_track(x, sample_rate=SR, hop=512, bpm=bpm, **c), rhythm_tables)


PAIRS = [(5, Sequence.TILE_ROWS + 1, 2 * Sequence.TILE_COLS + 3, "tile"), (5, Sequence.TILE_ROWS + 1, 2 * Sequence.TILE_COLS + 3, "general")]
SKEWED = dict(weights_add=(0, 0.5, 0.25), weights_mul=(2, 1, 1))


def pair(p, seed):
    d, n, m, route = p
    return [sig(seed, 2, d, n), sig(seed + 100, 2, d, m)], FAST_OFF if route == "general" else None


@row("smx_cost_matrix_hbm_f32", params=PAIRS)
def cost_matrix(p):
    xy, env = pair(p, 59)
    return Case(xy, lambda c, s, x, y: S.cost_matrix(x, y, metric="cosine"), env=env)


@row("smx_dtw_hbm_f32", params=PAIRS)
def dtw(p):
    xy, env = pair(p, 60)
    return Case(xy, lambda c, s, x, y: S.dtw(x, y, subseq=True, **SKEWED), env=env)


@row("smx_dtw_distance_hbm_f32", params=PAIRS)
def dtw_distance(p):
    xy, env = pair(p, 61)
    return Case(xy, lambda c, s, x, y: S.dtw_distance(x, y, **SKEWED), env=env)


FACTORS = [(33, 37, 3, "frobenius", "tile"), (33, 37, 3, "kullback-leibler", "tile"), (33, 37, 3, "frobenius", "general"), (70, 45, 33, "kullback-leibler", "tile")]


def factors(p, seed):
    F, T, K, beta, route = p
    return [mags(seed, 2, F, T), mags(seed + 1, 2, F, K), mags(seed + 2, 2, K, T)], beta, FAST_OFF if route == "general" else None


@row("smx_nmf_vram_f32", params=FACTORS)
def nmf(p):
    vwh, beta, env = factors(p, 62)
    return Case(vwh, lambda c, s, v, w, h: S.nmf(v, p[2], n_iter=5, beta=beta, W0=w, H0=h), env=env)        # five rounds: the H and W updates alternate


@row("smx_nmf_activations_vram_f32", params=FACTORS)
def nmf_activations(p):
    vwh, beta, env = factors(p, 65)
    return Case(vwh, lambda c, s, v, w, h: S.nmf_activations(v, w, n_iter=5, beta=beta, H0=h), env=env)


@row("smx_nmf_reconstruct_vram_f32", params=[(33, 37, 3, "all"), (33, 37, 3, "mask"), (70, 45, 33, "all")])
def nmf_reconstruct(p):
    F, T, K, what = p
    w, h = mags(68, 2, F, K), mags(69, 2, K, T)
    if what == "mask":
        return Case([w, h], lambda c, s, w_, h_: Decompose.mask(w_, h_, [0, 2]))
    return Case([w, h], lambda c, s, w_, h_: S.nmf_reconstruct(w_, h_))


@row("smx_nmf_divergence_vram_f32", params=FACTORS[:2])
def nmf_divergence(p):
    vwh, beta, env = factors(p, 70)
    return Case(vwh, lambda c, s, v, w, h: S.nmf_divergence(v, w, h, beta=beta), env=env)


# ---- rows: the streaming stages (three unequal chunks, then the flush) ------------------------------------------------------

@row("smx_stft_kernel_step_dev", "smx_stft_kernel_flush_dev", cold=True, params=[(256, 64), (2048, 512)])
def stft_kernel(p):
    n = p[1] * 47
    cuts = [0, n // 5, n // 5 * 3 + 1, n]
    return Case([sig(73, 2, n)], lambda c, k, x: streamed(k, x, cuts), lambda cold: stft_config(*p, cold),
                lambda c: Stft.Kernel.prepare(c, np.float32, 2, n))


@row("smx_stft_synthesis_step_dev", "smx_stft_synthesis_flush_dev", cold=True, params=[(256, 64), (2048, 512)])
def stft_synthesis(p):
    return Case([spectrum(74, 2, p[0] // 2 + 1, 30)], lambda c, k, z: streamed(k, z, [0, 7, 19, 30]), lambda cold: stft_config(*p, cold),
                lambda c: Stft.Synthesis.prepare(c, np.complex64, 2, 12))


@row("smx_cqt_kernel_step_f32_dev", "smx_cqt_kernel_flush_f32_dev", cold=True)
def cqt_kernel():
    return Case([sig(75, 2, 4096)], lambda c, k, x: streamed(k, x, [0, 1300, 3100, 4096]), lambda cold: cqt_config(36, cold),
                lambda c: Cqt.Kernel.prepare(c, channels=2, max_block=4096))


def to_device(k):
    return k.flush(device="cuda")


@row("smx_resample_kernel_step_f32_dev", "smx_resample_kernel_flush_f32_dev", cold=True)
def resample_kernel():
    return Case([sig(76, 2, 9001)], lambda c, k, x: streamed(k, x, [0, 2500, 6500, 9001], to_device), stage_x2, lambda c: Resample.Kernel.prepare(c, 2, 4000))


@row("smx_resample_stream_step_f32_dev", "smx_resample_stream_flush_f32_dev", cold=True)
def resample_stream():
    return Case([sig(77, 2, 9001)], lambda c, k, x: streamed(k, x, [0, 2500, 6500, 9001], to_device), lambda cold: resample_config((5, 7), cold, "direct"),
                lambda c: Resample.Kernel.prepare(c, 2, 4000))


@row("smx_energy_frames_device_f32", params=["rms", "zcr"])
def energy_stage(which):
    make = (lambda c: Energy.rms_stage(200, 64)) if which == "rms" else (lambda c: Energy.zero_crossing_rate_stage(200, 64))
    return Case([sig(78, 2, 3000)], lambda c, k, x: streamed(k, x, [0, 500, 1700, 3000]), state=make)


@row("smx_yin_frames_resident_f32")
def yin_stage():
    return Case([sig(79, 2, 3000)], lambda c, k, x: streamed(k, x, [0, 500, 1700, 3000]), state=lambda c: S.yin_stage(100.0, 1000.0, sample_rate=8000, frame_length=200, hop=64))


# ---- the tests -------------------------------------------------------------------------------------------------------------

IDS = [r.id for r in ROWS]


@pytest.mark.parametrize("r", ROWS, ids=IDS)
def test_fence(hold, r):
    """warm: the bits of the default stream, the caller's handle in every entry, the declared entries, and the synchronisation law"""
    case = r.case()
    cfg = case.make(False)
    want = ordinary(case, cfg, case.inputs)
    state = case.state(cfg)
    kept = []
    if state is not None:       # a streaming object is warm on its second pass over the same chunk sizes
        out, _, _ = fenced(hold, case, cfg, state, case.inputs, r.entries)
        same_bits(out, want, r.id + " (first pass)")
        kept.append(out)
        state.reset()
    out, pending, dt = fenced(hold, case, cfg, state, case.inputs, r.entries)
    same_bits(out, want, r.id)
    assert pending == (not r.synchronises), "%s %s (it came back after %.1f ms of a %g ms hold)" % (
        r.id, "synchronised the caller's stream" if not pending else "is declared to synchronise and did not", 1e3 * dt, H_MS)
    if not r.synchronises:
        assert 1e3 * dt <= H_MS / 2, "%s took %.1f ms to return, warm: it builds tables per call or waits for the device" % (r.id, 1e3 * dt)


TWICE = [r for r in ROWS if r.id in ("chroma_apply", "mfcc-2048-512", "power_to_db-80.0", "griffin_lim-100-25-False", "hpss-256-64-(31,31)", "cqt_transform-36-4096",
                                     "pyin-256-64-1500-8000-400.0-500.0", "time_stretch-0.75")]


@pytest.mark.parametrize("r", TWICE, ids=[r.id for r in TWICE])
def test_two_calls_in_a_row_stay_pending(hold, r):
    """the second call on a stream that is still held takes the scratch the first one gave back: it must not wait for the first
    one's release to run on the device (the runtime's hipFreeAsync does; the library's pool keeps such scratch per stream)"""
    case = r.case()
    twice = Case(case.inputs, lambda c, s, *xs: (case.call(c, s, *xs), case.call(c, s, *xs))[1], case.make, case.state, case.env)
    cfg = case.make(False)
    want = ordinary(case, cfg, case.inputs)
    out, pending, dt = fenced(hold, twice, cfg, None, case.inputs, r.entries)
    same_bits(out, want, r.id)
    assert pending and 1e3 * dt <= H_MS / 2, "%s twice: pending %s, back after %.1f ms of a %g ms hold" % (r.id, pending, 1e3 * dt, H_MS)


COLD = [r for r in ROWS if r.cold]


@pytest.mark.parametrize("r", COLD, ids=[r.id for r in COLD])
def test_cold_first_use(hold, r):
    """the first launch of a fresh configuration, table builds included, with the side stream current: bits only"""
    case = r.case()
    cfg = case.make(True)
    out, _, _ = fenced(hold, case, cfg, case.state(cfg), case.inputs, r.entries)
    same_bits(out, ordinary(case, cfg, case.inputs), r.id)


@pytest.mark.parametrize("r", ROWS, ids=IDS)
def test_two_streams(hold, r):
    """one configuration, data A on one stream and B on another, both held, both calls queued: each gets its own bits"""
    import torch
    case = r.case()
    cfg = case.make(False)
    data = [case.inputs, [other(a) for a in case.inputs]]
    want = [ordinary(case, cfg, d) for d in data]
    sides = [torch.cuda.Stream(), torch.cuda.Stream()]
    assert sides[0].cuda_stream != 0 and sides[1].cuda_stream not in (0, sides[0].cuda_stream)
    placed = [Placed(s, d) for s, d in zip(sides, data)]
    states = [case.state(cfg) for _ in sides]
    for p in placed:
        p.hold(hold, H_MS)
    got = [p.run(case, cfg, st)[0] for p, st in zip(placed, states)]
    for s in sides:
        s.synchronize()
    for k in (0, 1):
        same_bits(got[k], want[k], "%s on stream %d of two" % (r.id, k))


def test_envelope_cache_eviction_between_streams(hold):
    """two frame counts inverted alternately on two streams of one configuration; between the rounds 64 other counts go through the
    second stream, so the cache (64 envelopes) drops the tables of launches still queued behind the holds and the next round builds
    them again (smx_internal.hpp: the envelope's `owner`)"""
    import torch
    c = stft_config(2048, 512)
    counts = (24, 31)
    z = [spectrum(80 + f, 2, 1025, f) for f in counts]
    want = [ordinary(Case([a], lambda c_, s, t: Stft.invert(c_, t)), c, [a]) for a in z]
    others = [device(spectrum(f, 1, 1025, f)) for f in range(70, 70 + 64)]
    sides = [torch.cuda.Stream(), torch.cuda.Stream()]
    placed = [Placed(s, [a]) for s, a in zip(sides, z)]
    for p in placed:
        p.hold(hold, H_MS)
    got = [[], []]
    for round_ in range(3):
        for k, p in enumerate(placed):
            with torch.cuda.stream(p.side):
                got[k].append(Stft.invert(c, p.xs[0]))
        if round_ == 0:
            with torch.cuda.stream(sides[1]):
                for t in others:
                    t.record_stream(sides[1])
                    Stft.invert(c, t)
    for s in sides:
        s.synchronize()
    for k in (0, 1):
        for out in got[k]:
            same_bits([out], want[k], "invert of %d frames on stream %d" % (counts[k], k))


def test_a_wrong_stream_launch_reads_the_decoy(hold):
    """the fence bites: one single-launch entry given the DEFAULT stream's handle while the true input waits behind the hold on the
    side stream computes on the decoy.  All memory is valid; this only shows that a wrong-stream launch is visible."""
    import torch
    x, y = sig(90, 2, 5, 33), sig(91, 2, 5, 47)
    case = Case([x, y], lambda c, s, a, b: S.cost_matrix(a, b))
    want_true = ordinary(case, None, [x, y])
    want_decoy = ordinary(case, None, [decoy(x), decoy(y)])
    assert not torch.equal(bits(want_true[0]), bits(want_decoy[0]))
    side = torch.cuda.Stream()
    assert side.cuda_stream != 0 and torch.cuda.default_stream().cuda_stream == 0
    p = Placed(side, [x, y])
    out = torch.empty_like(want_true[0])
    torch.cuda.synchronize()
    p.hold(hold, H_MS)
    a, b = p.xs
    check(lib.smx_cost_matrix_hbm_f32(C.c_void_p(a.data_ptr()), C.c_void_p(b.data_ptr()), 2, 5, 33, 47, 33, 47, 0, C.c_void_p(out.data_ptr()), C.c_void_p(0)))
    torch.cuda.default_stream().synchronize()
    assert not side.query(), "the hold ended before the wrong-stream launch did"
    got = out.clone()
    side.synchronize()
    torch.cuda.synchronize()
    same_bits([got], want_decoy, "the launch on the default stream")
    assert torch.equal(a, p.true[0]) and torch.equal(b, p.true[1])      # the true inputs did arrive, behind the hold


def test_synchronize_drains_its_stream_alone(hold):
    """smx_synchronize(stream) returns once that stream is idle and leaves another held stream pending"""
    import torch
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    x = torch.zeros(16, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(s2):
        hold(4 * H_MS)
        x.add_(1)
    with torch.cuda.stream(s1):
        hold(H_MS / 2)
    assert not s1.query()
    check(lib.smx_synchronize(C.c_void_p(s1.cuda_stream)))
    assert s1.query() and not s2.query()
    s2.synchronize()


def test_coverage_law():
    """every function of the header whose parameters end in `void *stream)` runs in a row above, or is a diagnostic face, or
    smx_synchronize with its own test (no GPU work)"""
    declared = set(STREAM_ENTRIES)
    assert len(declared) >= 80
    for name in EXCLUDED:
        assert name in declared and (name.startswith("smx_debug_") or name == "smx_synchronize"), name
    assert not set(TABLE) & set(EXCLUDED)
    missing = sorted(declared - set(TABLE) - set(EXCLUDED))
    assert not missing, "stream-taking entry points without a row: %s" % ", ".join(missing)
    unknown = sorted((set(TABLE) | set(EXCLUDED)) - declared)
    assert not unknown, "rows for entry points the header does not declare: %s" % ", ".join(unknown)
    for r in ROWS:
        assert r.entries and r.entries <= declared, r.id
    assert len(set(IDS)) == len(IDS)


def host_return_times(repeats=3):
    """[(row id, the largest host-side return in ms of `repeats` warm calls on the default stream)]: what H_MS is chosen from"""
    import torch
    rows = []
    for r in ROWS:
        case = r.case()
        cfg = case.make(False)
        xs = [device(a) for a in case.inputs]
        worst, state = 0.0, case.state(cfg)
        with environment(case.env):
            for k in range(repeats + 1):
                if state is not None:
                    state.reset()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                case.call(cfg, state, *xs)
                dt = time.perf_counter() - t0
                torch.cuda.synchronize()
                worst = max(worst, dt) if k else 0.0
        rows.append((r.id, 1e3 * worst))
    return rows
