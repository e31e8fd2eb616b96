"""Effects on the device (soundml_amd/csrc/effects.hip) against the numpy restatement of effects.ml
(tests/effects_restatement.py, itself pinned to the reference's golden vectors by tests/test_effects_restatement.py), the
composition and batch laws bit for bit, and the golden vectors themselves under the float64 interior.

The vocoder is float64 inside at every interior setting, so it is compared pointwise on the same spectrum: complex128 at
the reference's own 1e-11, complex64 at four float32 rounding steps of the peak against the restatement rounded to
complex64.  ``time_stretch`` under the float32 interior feeds the STFT's 1e-7 differences back into every later phase (up
to 2.9e4 x, pvoc_goldens.ml:33-43), so that path is checked by the laws, not against the golden vectors."""
import functools

import numpy as np
import pytest

import soundml_amd as S
from soundml_amd import Effects, Resample, Stft
from conftest import F32_ATOL, F32_RTOL, check_close
from oracle import soundml_oracle as O

import effects_restatement as R

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

PHASES = ["independent", "locked"]
# (fft, hop, frames).  The independent kernel takes 32 output frames and at most 48 analysis frames per chunk: 130 frames
# are several chunks at every rate (36 output frames at rate 3.7, 390 at 1/3), so the accumulator is carried across chunks;
# 37 frames are one analysis chunk at the high rates and several at the low ones.  fft 31 has 16 bins (half a bin block),
# fft 2048 has 1025 (32 blocks and one bin).
GEOMETRIES = [(2048, 512, 37), (2048, 512, 130), (64, 16, 9), (31, 5, 26), (256, 64, 1), (256, 64, 0)]
RATES = [0.5, 0.75, 1.0, 1.25, 1.37, 2.0, 3.7, 1.0 / 3.0]
LEADS = [(), (3,), (2, 3)]


@pytest.fixture(autouse=True)
def _default_interior():
    S.set_interior("float32")
    yield
    S.set_interior("float32")


def dev(a):
    return torch.from_numpy(np.array(a, copy=True, order="C")).to("cuda:0")


def host(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)


def config(fft, hop):
    return Stft.Config.create(fft_size=fft, hop=hop, pad=("constant", 0.0))


@functools.lru_cache(maxsize=None)
def noise_spectrum(bins, frames):
    """LCG noise, complex128 [2; 3; bins; frames]: one stream for the first signal, the others its bins rotated and scaled by
    powers of two (still LCG noise, and no two magnitudes of a frame tie)."""
    base = O.lcg_signal(2 * bins * frames, R.GOLDEN_SEED).reshape(2, bins, frames)
    base = base[0] + 1j * base[1]
    z = np.stack([np.roll(base, 7 * s, axis=0) * (2.0 ** -s) for s in range(6)]).reshape(2, 3, bins, frames)
    z.setflags(write=False)
    return z


@functools.lru_cache(maxsize=None)
def noise_parts(bins, frames, single):
    """The spectrum (rounded to complex64 for ``single``) with its magnitudes and arguments, which every rate and phase mode
    shares."""
    z = noise_spectrum(bins, frames)
    if single:
        z = z.astype(np.complex64)
    return z, R.polar(z)


@functools.lru_cache(maxsize=None)
def restated(fft, hop, frames, rate, phase, single):
    """The restatement on the whole [2; 3] stack, once: the lead shapes below are its slices (every signal is vocoded on its
    own).  single: on the spectrum rounded to complex64, the result rounded to complex64."""
    z, parts = noise_parts(fft // 2 + 1, frames, single)
    y = R.vocode(fft, hop, z, rate, locked=phase == "locked", parts=parts)
    y = y.astype(np.complex64) if single else y
    y.setflags(write=False)
    return y


def take(a, lead):
    return a[(0,) * (2 - len(lead))]


def deviation(got, want, what):
    """(worst |d|, bound): complex128 at 1e-11 * max(1, peak |Y|), complex64 at 2**-22 * peak |Y|; shapes and dtypes equal."""
    got = host(got)
    assert got.shape == want.shape and got.dtype == want.dtype, what
    if want.size == 0:
        return 0.0, 0.0
    peak = float(np.max(np.abs(want)))
    bound = 2.0 ** -22 * peak if want.dtype == np.complex64 else 1e-11 * max(1.0, peak)
    return float(np.max(np.abs(got.astype(np.complex128) - want.astype(np.complex128)))), bound


def check_vocoded(got, want, what):
    worst, bound = deviation(got, want, what)
    assert worst <= bound, "%s: worst |d| %.3g, bound %.3g" % (what, worst, bound)


# ---- 1. the vocoder against the restatement on the same spectrum -----------------------------------------------------------
@pytest.mark.parametrize("phase", PHASES)
@pytest.mark.parametrize("geometry", GEOMETRIES, ids=lambda g: "fft%d_hop%d_frames%d" % g)
def test_vocoder_against_the_restatement(geometry, phase):
    """Every rate, lead shape, dtype and face of one geometry and phase mode; every miss is listed before the assertion.

    The bound leaves no room for an argument that differs in its last bit: the phases reach 2e5 rad after 111 output frames
    and 6e5 rad after 390 (ulp 2.9e-11 and 1.2e-10), and an argument one ulp (2e-16) apart moves ``omega + deviation`` across
    a rounding boundary once in a thousand steps.  So both sides round the argument as the reference's libm does: the
    restatement calls libm's atan2 (``R.polar``), the kernel evaluates it in double-double and rounds once (atan2_dd.hpp)."""
    fft, hop, frames = geometry
    c = config(fft, hop)
    z128 = noise_spectrum(fft // 2 + 1, frames)
    z64 = z128.astype(np.complex64)
    misses = []
    for rate in RATES:
        for lead in LEADS:
            for z, single in ((z128, False), (z64, True)):
                want = take(restated(fft, hop, frames, rate, phase, single), lead)
                arg = np.ascontiguousarray(take(z, lead))
                what = "fft %d hop %d frames %d rate %g %s lead %s %s" % (fft, hop, frames, rate, phase, lead, arg.dtype)
                out = Effects.phase_vocoder(c, dev(arg), rate, phase=phase)
                assert out.is_cuda
                for face, got in (("host", Effects.phase_vocoder(c, arg, rate, phase=phase)), ("device", out)):
                    worst, bound = deviation(got, want, what + " " + face)
                    if worst > bound:
                        misses.append("%s %s: worst |d| %.3g, bound %.3g" % (what, face, worst, bound))
    print("\n".join(misses))
    assert not misses, "%d of %d comparisons miss their bound:\n%s" % (len(misses), 2 * 2 * len(RATES) * len(LEADS), "\n".join(misses))


@pytest.mark.parametrize("phase", PHASES)
def test_vocoder_through_a_silent_frame(phase):
    """An all-zero analysis frame in the middle, with every combination of signed zeros (arg(-0 + 0i) = pi, arg(-0 - 0i) =
    -pi, as numpy and OCaml have it; no peaks there, so the locked phases are left alone), followed by signal."""
    fft, hop, frames = 64, 16, 9
    c = config(fft, hop)
    z = noise_spectrum(fft // 2 + 1, frames)[0, 0].copy()
    signs = np.array([0.0, -0.0])
    k = np.arange(z.shape[0])
    z[:, 4] = signs[k % 2] + 1j * signs[(k // 2) % 2]
    for rate in (0.5, 0.75, 1.0, 1.37, 2.0):
        want = R.vocode(fft, hop, z, rate, locked=phase == "locked")
        check_vocoded(Effects.phase_vocoder(c, z, rate, phase=phase), want, "silent frame, rate %g, complex128" % rate)
        check_vocoded(Effects.phase_vocoder(c, dev(z), rate, phase=phase), want, "silent frame, rate %g, complex128 device" % rate)
        z64 = z.astype(np.complex64)
        want = R.vocode(fft, hop, z64, rate, locked=phase == "locked").astype(np.complex64)
        check_vocoded(Effects.phase_vocoder(c, z64, rate, phase=phase), want, "silent frame, rate %g, complex64" % rate)


def test_locked_vocoder_with_more_bins_than_the_default_lds_grant():
    """fft 4096: 2049 bins hold 82 KB of rows, past the 64 KB a kernel gets unasked."""
    fft, hop, frames = 4096, 1024, 5
    z = noise_spectrum(fft // 2 + 1, frames)[0, 0]
    want = R.vocode(fft, hop, z, 0.75, locked=True)
    check_vocoded(Effects.phase_vocoder(config(fft, hop), z, 0.75, phase="locked"), want, "fft 4096 locked")


# ---- 2. rate 1 --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("phase", PHASES)
def test_rate_one_is_the_identity_on_spectra(phase):
    """At rate 1 the accumulator follows the analysis phase up to whole turns and the magnitudes are the input's."""
    z = noise_spectrum(1025, 130).astype(np.complex64)
    got = host(Effects.phase_vocoder(config(2048, 512), dev(z), 1.0, phase=phase))
    peak = float(np.max(np.abs(z)))
    assert got.shape == z.shape and got.dtype == np.complex64
    assert float(np.max(np.abs(got.astype(np.complex128) - z.astype(np.complex128)))) <= 2.0 ** -22 * peak


# ---- 3. composition, bit for bit, under both interiors --------------------------------------------------------------------------
SIZES = [(256, 64, 4000), (2048, 512, 20000)]
RATIOS = [(3, 2), (1, 2), "semitones(4)", (1, 1)]


def audio(shape, dtype=np.float32, seed=7):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, shape).astype(dtype)


def ratio_of(r):
    return Effects.semitones(4) if isinstance(r, str) else r


def composed_stretch(c, x, rate, phase, interior):
    """Stft.invert(c, phase_vocoder(c, Stft.transform(c, x), rate), length); under the float64 interior float32 audio is
    widened first and the result rounded once."""
    widen = interior == "float64" and (x.dtype == np.float32 if isinstance(x, np.ndarray) else x.dtype == torch.float32)
    wide = (x.astype(np.float64) if isinstance(x, np.ndarray) else x.double()) if widen else x
    length = R.stretch_length(int(x.shape[-1]), rate)
    y = Stft.invert(c, Effects.phase_vocoder(c, Stft.transform(c, wide), rate, phase=phase), length=length)
    if widen:
        y = y.astype(np.float32) if isinstance(y, np.ndarray) else y.float()
    return y


@pytest.mark.parametrize("interior", ["float32", "float64"])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "fft%d_hop%d_n%d" % s)
def test_time_stretch_is_its_three_stages(size, interior):
    fft, hop, n = size
    c = config(fft, hop)
    S.set_interior(interior)
    try:
        for r in RATIOS:
            num, den = ratio_of(r)
            rate = float(den) / float(num)
            for phase in PHASES:
                for x in (audio((2, n)), audio((2, n), np.float64), dev(audio((2, n)))):
                    got = Effects.time_stretch(c, x, rate, phase=phase)
                    want = composed_stretch(c, x, rate, phase, interior)
                    what = "%s %s rate %g %s %s" % (size, interior, rate, phase, x.dtype)
                    assert got.dtype == x.dtype and tuple(got.shape) == (2, R.stretch_length(n, rate)), what
                    assert np.array_equal(host(got), host(want)), what
    finally:
        S.set_interior("float32")


@pytest.mark.parametrize("interior", ["float32", "float64"])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "fft%d_hop%d_n%d" % s)
def test_pitch_shift_is_stretch_then_resample(size, interior):
    fft, hop, n = size
    c = config(fft, hop)
    S.set_interior(interior)
    try:
        for r in RATIOS:
            num, den = ratio_of(r)
            resampler = Resample.Config.create(num, den)
            for phase in PHASES:
                for x in (audio((2, n)), dev(audio((2, n))), audio((2, n), np.float64)):
                    got = Effects.pitch_shift(c, x, (num, den), phase=phase)
                    stretched = Effects.time_stretch(c, x, float(den) / float(num), phase=phase)
                    if x.dtype == np.float64:   # the documented deviation: the conversion runs in float32
                        stretched = stretched.astype(np.float32)
                    y = host(Resample.apply(resampler, stretched))
                    want = np.zeros((2, n), y.dtype)
                    kept = min(n, y.shape[-1])
                    want[:, :kept] = y[:, :kept]
                    what = "%s %s ratio %d/%d %s %s" % (size, interior, num, den, phase, x.dtype)
                    assert got.dtype == x.dtype and tuple(got.shape) == (2, n), what
                    assert np.array_equal(host(got), want.astype(host(got).dtype)), what
    finally:
        S.set_interior("float32")


# ---- 4. batch law -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("phase", PHASES)
def test_a_batch_is_its_slices(phase):
    fft, hop, n = 256, 64, 4000
    c = config(fft, hop)
    x = audio((2, 3, n))
    z = noise_spectrum(fft // 2 + 1, 37).astype(np.complex64)
    calls = [("phase_vocoder", lambda a: Effects.phase_vocoder(c, a, 1.37, phase=phase), z, 2),
             ("time_stretch", lambda a: Effects.time_stretch(c, a, 0.75, phase=phase), x, 1),
             ("pitch_shift", lambda a: Effects.pitch_shift(c, a, (3, 2), phase=phase), x, 1)]
    for name, call, arg, core in calls:
        for place in (lambda a: np.ascontiguousarray(a), dev):
            whole = host(call(place(arg)))
            assert whole.shape[:2] == (2, 3)
            for i in range(2):
                for j in range(3):
                    assert np.array_equal(whole[i, j], host(call(place(arg[i, j])))), (name, i, j)


# ---- 5. the reference's golden vectors under the float64 interior ---------------------------------------------------------------
def replay(case, got, fraction=None):
    p = case["params"]
    got = host(got)
    assert got.dtype == np.dtype(p["dtype"])
    if fraction is not None:
        rtol, atol = 0.0, fraction * float(np.max(np.abs(case["values"])))
    elif p["dtype"] == "float64":
        rtol, atol = 0.0, R.FLOAT64_ATOL
    else:
        rtol, atol = F32_RTOL, F32_ATOL
    check_close(got, case["values"], shape=case["shape"], rtol=rtol, atol=atol, msg=case["name"])


def golden_stretch(case, phase):
    p = case["params"]
    S.set_interior("float64")
    try:
        got = Effects.time_stretch(config(p["fft_size"], p["hop"]), R.golden_signal(p), p["rate"], phase=phase)
    finally:
        S.set_interior("float32")
    replay(case, got)


@pytest.mark.parametrize("case", R.golden_cases("stretch"))
def test_stretch_goldens(case):
    golden_stretch(case, "independent")


@pytest.mark.parametrize("case", R.golden_cases("pitchstretch"))
def test_pitchstretch_goldens(case):
    assert float(case["params"]["den"]) / float(case["params"]["num"]) == case["params"]["rate"]
    golden_stretch(case, "independent")


@pytest.mark.parametrize("case", R.golden_cases("locked"))
def test_locked_goldens(case):
    golden_stretch(case, "locked")


@pytest.mark.parametrize("interior", ["float32", "float64"])
@pytest.mark.parametrize("case", R.golden_cases("pitch"))
def test_pitch_goldens(case, interior):
    p = case["params"]
    S.set_interior(interior)
    try:
        got = Effects.pitch_shift(config(p["fft_size"], p["hop"]), R.golden_signal(p), (p["num"], p["den"]))
    finally:
        S.set_interior("float32")
    replay(case, got, fraction=R.PITCH_FRACTION)


# ---- 6. lengths and errors --------------------------------------------------------------------------------------------------
def test_lengths_and_empty_signals():
    c = config(64, 16)
    for n in (0, 1, 127, 1000):
        for rate in (0.5, 1.37, 2.0):
            want = int(np.rint(n / rate))
            for x in (audio((n,)), audio((2, n), np.float64), dev(audio((3, n)))):
                y = Effects.time_stretch(c, x, rate)
                assert y.shape[-1] == want and tuple(y.shape[:-1]) == tuple(x.shape[:-1]) and y.dtype == x.dtype
                assert np.isfinite(host(y)).all()
    for x in (audio((0,)), dev(audio((2, 0)))):
        assert Effects.time_stretch(c, x, 1.37).shape == x.shape
        assert Effects.pitch_shift(c, x, (3, 2)).shape == x.shape
    z = np.zeros((2, 33, 0), np.complex64)
    assert Effects.phase_vocoder(c, z, 0.5).shape == (2, 33, 0) and Effects.phase_vocoder(c, dev(z), 0.5, phase="locked").shape == (2, 33, 0)
    assert host(Effects.pitch_shift(c, dev(audio((2, 300))), (1, 1))).shape == (2, 300)


def test_errors_on_device_tensors():
    c = config(64, 16)
    x = dev(audio((2, 500)))
    z = dev(noise_spectrum(33, 9).astype(np.complex64))
    cases = [
        (lambda: Effects.phase_vocoder(c, z, 0.0), "phase_vocoder: cannot stretch by a rate of 0 (the rate must be finite and positive)"),
        (lambda: Effects.phase_vocoder(c, z, float("nan")), "phase_vocoder: cannot stretch by a rate of nan (the rate must be finite and positive)"),
        (lambda: Effects.phase_vocoder(c, z[0, 0, :, 0], 1.5), "phase_vocoder: cannot vocode a rank-1 tensor (the bin and frame axes must exist)"),
        (lambda: Effects.phase_vocoder(c, z[:, :, :32], 1.5),
         "phase_vocoder: cannot vocode 32 frequency bins of a 64-point transform (the bin axis must hold fft_size / 2 + 1 = 33 values)"),
        (lambda: Effects.time_stretch(c, x, float("inf")), "time_stretch: cannot stretch by a rate of inf (the rate must be finite and positive)"),
        (lambda: Effects.time_stretch(c, x[0, 0], 1.5), "time_stretch: cannot process a rank-zero tensor (the time axis must exist)"),
        (lambda: Effects.pitch_shift(c, x, (0, 1)), "pitch_shift: cannot shift by a frequency ratio of 0/1 (both terms must be at least 1)"),
        (lambda: Effects.pitch_shift(c, x[0, 0], (3, 2)), "pitch_shift: cannot process a rank-zero tensor (the time axis must exist)"),
    ]
    for call, message in cases:
        with pytest.raises(S.InvalidArgument) as e:
            call()
        assert str(e.value) == message
    gaps = Stft.Config.create(fft_size=64, hop=64)   # fails Stft.nola
    for call in (lambda: Effects.time_stretch(gaps, x, 1.5), lambda: Effects.pitch_shift(gaps, x, (3, 2))):
        with pytest.raises(S.InvalidArgument) as e:
            call()
        with pytest.raises(S.InvalidArgument) as inv:
            Stft.invert(gaps, torch.zeros((2, 33, 9), dtype=torch.complex64, device="cuda:0"), length=333)
        assert str(e.value) == str(inv.value)
