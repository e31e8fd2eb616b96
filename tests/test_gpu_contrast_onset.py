"""Spectral contrast and onset strength on the device against the reference's golden vectors and the numpy restatement
(tests/contrast_onset_restatement.py, itself pinned to the goldens by test_contrast_onset_restatement.py).

"1 ulp32 + 1e-11" below is |got - want64| <= ulp_float32(want64) + 1e-11.  The relative term is the one output rounding.  The
absolute term: two float64 logarithms good to 1.5e-14 give 1.3e-13 dB per band or mel, and a float64 sum of 128 terms of
magnitude <= 80 adds about 1e-12."""
import contextlib
import ctypes as C
import functools
import os

import numpy as np
import pytest

import soundml_amd as S
from soundml_amd import Mel, Stft, onset
from soundml_amd._lib import check, lib
from conftest import F32_ATOL, F32_RTOL, F64_ATOL, F64_RTOL, check_close, golden_cases
from oracle import soundml_oracle as O

import contrast_onset_restatement as R

pytestmark = pytest.mark.gpu

LOG64_ATOL, LOG32_RTOL, LOG32_ATOL = 1e-9, 1e-4, 1e-4      # onset_goldens.ml:24-32
ABS = 1e-11
SR = 22050


@pytest.fixture(autouse=True)
def _default_interior():
    S.set_interior("float32")
    yield
    S.set_interior("float32")


@contextlib.contextmanager
def general_path():
    """SMX_DISABLE_FAST: the bisection on the keys' bits for every take (the library reads it per call)"""
    saved = os.environ.get("SMX_DISABLE_FAST")
    os.environ["SMX_DISABLE_FAST"] = "1"
    try:
        yield
    finally:
        if saved is None:
            os.environ.pop("SMX_DISABLE_FAST", None)
        else:
            os.environ["SMX_DISABLE_FAST"] = saved


def dev(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()          # (a copy: the shared inputs are read-only)


def host(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)


def bits(a):
    a = np.ascontiguousarray(host(a))
    return a.view(np.int32 if a.dtype == np.float32 else np.int64)


def same_bits(a, b, what):
    a, b = bits(a), bits(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert np.array_equal(a, b), "%s: %d elements differ" % (what, int((a != b).sum()))


def ulp_gate(got, want64, absolute, what):
    assert host(got).dtype == np.float32, what
    excess = R.within_ulp32(host(got), want64, absolute)
    assert excess <= 0.0, "%s: %.3g beyond 1 ulp32 + %g" % (what, excess, absolute)


def check_fast(actual, expected, msg):
    """test_gpu_parity.check_fast: |a - e| <= 1e-5 peak + 1e-5 |e|"""
    a, e = np.asarray(actual, np.float64), np.asarray(expected, np.float64).reshape(np.shape(actual))
    peak = np.max(np.abs(e)) if e.size else 0.0
    bad = np.abs(a - e) > 1e-5 * peak + 1e-5 * np.abs(e)
    assert not bad.any(), "%s: %d/%d outside 1e-5 (max err %.3g, peak %.3g)" % (msg, int(bad.sum()), a.size, float(np.max(np.abs(a - e))), peak)


# ---- goldens ----------------------------------------------------------------------------------------------------------------

def golden_input(p):
    c = Stft.Config.create(fft_size=p["fft_size"], hop=p["hop"], alignment=p["alignment"])
    return c, R.signal(p["length"], envelope=p["envelope"], silence_tail=p["silence_tail"]).astype(p["dtype"])


def golden_check(case, face, linear):
    """host arrays in the case's dtype; float32 cases also on device tensors, under the float64 interior at the reference's
    tolerances and under the default interior at 1e-4 / 1e-4 (logarithmic) or 1e-5 of the peak (linear)"""
    p = case["params"]
    if p["dtype"] == "float64":
        got = face(lambda a: a)
        assert got.dtype == np.float64
        check_close(got, case["values"], case["shape"], F64_RTOL, F64_ATOL if linear else LOG64_ATOL, case["name"])
        return
    for place in (lambda a: a, dev):
        S.set_interior("float64")
        got = host(face(place))
        assert got.dtype == np.float32
        rtol, atol = (F32_RTOL, F32_ATOL) if linear else (LOG32_RTOL, LOG32_ATOL)
        check_close(got, case["values"], case["shape"], rtol, atol, case["name"] + "/float64 interior")
        S.set_interior("float32")
        got = host(face(place))
        assert list(got.shape) == list(case["shape"])
        if linear:
            check_fast(got, case["values"], case["name"])
        else:
            check_close(got, case["values"], case["shape"], LOG32_RTOL, LOG32_ATOL, case["name"] + "/float32 interior")


@pytest.mark.parametrize("case", golden_cases("onset", "spectral_contrast"))
def test_contrast_goldens(case):
    p = case["params"]
    c, x = golden_input(p)
    golden_check(case, lambda place: S.spectral_contrast(c, place(x), sample_rate=p["sample_rate"], n_bands=p["n_bands"], f_min=p["f_min"],
                                                         quantile=p["quantile"], linear=p["linear"]), p["linear"])


@pytest.mark.parametrize("case", golden_cases("onset", "onset_strength"))
def test_onset_goldens(case):
    p = case["params"]
    c, x = golden_input(p)
    mc = Mel.Config.create(n_mels=p["n_mels"], sample_rate=p["sample_rate"], fft_size=p["fft_size"])
    golden_check(case, lambda place: S.onset_strength(c, mc, place(x), lag=p["lag"]), False)


# ---- selection --------------------------------------------------------------------------------------------------------------

PLANE = (3, 1025, 70)          # one full 64-frame tile and a ragged one
SELECTION = [(SR, 0.02), (SR, 0.0375), (SR, 0.04), (SR, 0.5), (SR, 0.97), (48000, 0.02)]     # top-band takes 9, 16, 17, 216, 418; 15


@functools.lru_cache(maxsize=None)
def tied_plane():
    """uniform values on 12 levels, so ties are everywhere; one all-zero frame, one all-equal frame"""
    rng = np.random.default_rng(20260802)
    s = (rng.integers(0, 12, size=PLANE) / 11.0).astype(np.float32)
    s[0, :, 5] = 0.0
    s[1, :, 67] = 0.5
    s.setflags(write=False)
    return s


@functools.lru_cache(maxsize=None)
def tied_means(sample_rate, quantile):
    bands = R.plan(6, 200.0, quantile, sample_rate, 2048)
    return bands, R.means(tied_plane(), bands)


def want_contrast(means, linear, clamped):
    valley, peak = means
    if linear:
        return peak - valley
    top_db = 80.0 if clamped else None
    return O.power_to_db(peak, top_db=top_db) - O.power_to_db(valley, top_db=top_db)


@pytest.mark.parametrize("sample_rate,quantile", SELECTION)
def test_selection(sample_rate, quantile):
    s = tied_plane()
    bands, means = tied_means(sample_rate, quantile)
    if (sample_rate, quantile) == (SR, 0.0375):
        assert bands[-1][2] == 16
    if (sample_rate, quantile) == (SR, 0.04):
        assert bands[-1][2] == 17          # the first take past the register lists
    kw = dict(sample_rate=sample_rate, quantile=quantile)
    stage = S.spectral_contrast_stage(Stft.Config.create(fft_size=2048, hop=512), **kw)
    sd, s64 = dev(s), s.astype(np.float64)
    linear = S.spectral_contrast_of_spectrogram(sd, linear=True, **kw)
    ulp_gate(linear, want_contrast(means, True, True), 0.0, ("linear", sample_rate, quantile))
    ulp_gate(S.spectral_contrast_of_spectrogram(sd, **kw), want_contrast(means, False, True), ABS, ("clamped", sample_rate, quantile))
    ulp_gate(stage.step(sd), want_contrast(means, False, False), ABS, ("unclamped", sample_rate, quantile))
    same_bits(S.spectral_contrast_of_spectrogram(s, linear=True, **kw), linear, "host float32 against the device tensor")
    for lin in (True, False):
        got = S.spectral_contrast_of_spectrogram(s64, linear=lin, **kw)
        assert got.dtype == np.float64
        check_close(got, want_contrast(means, lin, True), list(PLANE[:1]) + [7, PLANE[2]], 1e-9, 1e-9, "host float64")
    with general_path():
        same_bits(S.spectral_contrast_of_spectrogram(sd, linear=True, **kw), linear, "the general path against the register lists")
        ulp_gate(S.spectral_contrast_of_spectrogram(sd, **kw), want_contrast(means, False, True), ABS, "general, clamped")


def test_negative_or_nan_magnitudes_are_refused():
    """contrast.ml:246-251, the flat spectrogram face only; the stage does not look"""
    for bad in (-1.0, float("nan")):
        s = np.array(tied_plane())
        s[2, 700, 69] = bad
        for place in (lambda a: a, dev):
            with pytest.raises(S.InvalidArgument) as e:
                S.spectral_contrast_of_spectrogram(place(s), sample_rate=SR)
            assert str(e.value) == ("spectral_contrast_of_spectrogram: cannot analyse a spectrogram with negative or NaN values (a magnitude "
                                    "spectrogram is non-negative)")


def test_slice_law():
    """no whole-tensor maximum involved: row 1 of the three-clip call is the one-clip call bit for bit"""
    s = tied_plane()
    c = Stft.Config.create(fft_size=2048, hop=512)
    for quantile in (0.02, 0.5):
        faces = [lambda a: S.spectral_contrast_of_spectrogram(a, sample_rate=SR, quantile=quantile, linear=True),
                 lambda a: S.spectral_contrast_stage(c, sample_rate=SR, quantile=quantile).step(a),
                 lambda a: S.spectral_contrast_stage(c, sample_rate=SR, quantile=quantile, linear=True).step(a)]
        for place in (dev, lambda a: a, lambda a: a.astype(np.float64)):
            for face in faces:
                same_bits(host(face(place(s)))[1:2], face(place(s[1:2])), ("slice", quantile))
    db = noise_db((3, 40, 70))
    for place in (dev, lambda a: a, lambda a: a.astype(np.float64)):
        same_bits(host(onset.flux(place(db), 3))[1:2], onset.flux(place(db[1:2]), 3), "flux slice")


# ---- the whole-tensor clamp -------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def gated_pair():
    """two clips, the second 1e-3 times the first: a noise burst over a floor 120 dB under it"""
    rng = np.random.default_rng(7)
    gate = np.full(4000, 1e-6)
    gate[1500:2500] = 1.0
    x = rng.uniform(-1, 1, 4000) * gate
    pair = np.stack([x, 1e-3 * x]).astype(np.float32)
    pair.setflags(write=False)
    return pair


def test_whole_tensor_clamp_onset():
    x = gated_pair()
    c = Stft.Config.create(fft_size=512, hop=128)
    mc = Mel.Config.create(n_mels=40, sample_rate=SR, fft_size=512)
    xd = dev(x)
    batch, alone = host(S.onset_strength(c, mc, xd)), host(S.onset_strength(c, mc, xd[1:2]))
    mel = host(S.mel_spectrogram(c, mc, xd))
    ulp_gate(batch, R.envelope64(mel, 1, 2), ABS, "the batch")
    ulp_gate(alone, R.envelope64(mel[1:2], 1, 2), ABS, "the quiet clip alone")
    assert float(np.max(np.abs(batch[1] - alone[0]))) > 1.0        # 25 dB in the restatement on the CPU: the clamp sits under the LOUD clip's maximum
    same_bits(S.onset_strength(c, mc, x), batch, "host float32 against the device tensor")


def test_whole_tensor_clamp_contrast():
    x = gated_pair()
    c = Stft.Config.create(fft_size=512, hop=128)
    xd = dev(x)
    batch, alone = host(S.spectral_contrast(c, xd, sample_rate=SR)), host(S.spectral_contrast(c, xd[1:2], sample_rate=SR))
    mag = host(Stft.power_spectrum(c, xd, 1.0))
    bands = R.plan(6, 200.0, 0.02, SR, 512)
    ulp_gate(batch, R.contrast64(mag, bands), ABS, "the batch")
    ulp_gate(alone, R.contrast64(mag[1:2], bands), ABS, "the quiet clip alone")
    assert float(np.max(np.abs(batch[1] - alone[0]))) > 1.0        # 17 dB in the restatement on the CPU


# ---- flux -------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def noise_db(shape):
    db = np.random.default_rng(sum(shape)).uniform(-80.0, 0.0, size=shape).astype(np.float32)
    db.setflags(write=False)
    return db


@pytest.mark.parametrize("bins", [40, 1, 128])
def test_flux(bins):
    db = noise_db((3, bins, 70))
    dd = dev(db)
    for lag in (1, 3, 69, 70, 200):
        want = R.flux64(db, lag)
        got = onset.flux(dd, lag)
        assert tuple(got.shape) == (3, 70)
        ulp_gate(got, want, ABS, (bins, lag))
        if lag >= 70:
            assert not host(got).any()
        same_bits(onset.flux(db, lag), got, "host float32 against the device tensor")
        wide = onset.flux(db.astype(np.float64), lag)
        assert wide.dtype == np.float64
        check_close(wide, want, [3, 70], 1e-9, 1e-9, "host float64")


# ---- the audio faces --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kw,n,shift", [(dict(hop=128), 4000, 2), (dict(hop=300), 4000, 0), (dict(hop=128, alignment="left"), 4000, 0),
                                        (dict(hop=128, pad=("constant", 0.0)), 200, 2)])
def test_onset_strength_is_the_flux_of_the_device_mel(kw, n, shift):
    c = Stft.Config.create(fft_size=512, **kw)
    mc = Mel.Config.create(n_mels=40, sample_rate=SR, fft_size=512)
    xd = dev(np.random.default_rng(n + shift).uniform(-1, 1, size=(2, n)).astype(np.float32))
    mel = host(S.mel_spectrogram(c, mc, xd))
    frames = mel.shape[-1]
    for lag in (1, 3):
        got = S.onset_strength(c, mc, xd, lag=lag)
        assert tuple(got.shape) == (2, frames)
        ulp_gate(got, R.envelope64(mel, lag, shift), ABS, (kw, lag))
        if frames <= shift:
            assert n == 200 and not host(got).any()
        else:
            assert host(got).any()
    assert (n == 200) == (frames <= shift)


def test_contrast_of_audio_is_contrast_of_its_magnitudes():
    c = Stft.Config.create(fft_size=512, hop=128)
    x = np.random.default_rng(3).uniform(-1, 1, size=(2, 4000)).astype(np.float32)
    for place in (dev, lambda a: a):
        for linear in (False, True):
            same_bits(S.spectral_contrast(c, place(x), sample_rate=SR, linear=linear),
                      S.spectral_contrast_of_spectrogram(Stft.power_spectrum(c, place(x), 1.0), sample_rate=SR, linear=linear), linear)


# ---- stages -----------------------------------------------------------------------------------------------------------------

CUTS = [0, 1, 3, 5, 8, 12, 70]         # chunks of 1, 2, 2, 3, 4 frames and the rest


@pytest.mark.parametrize("where", ["host", "device"])
def test_onset_stage_partitions(where):
    import torch
    db = noise_db((3, 40, 70))
    place = dev if where == "device" else (lambda a: a)
    whole = onset.flux(place(db), 3)
    stage = S.onset_strength_stage(lag=3)
    for _ in range(2):
        parts = [stage.step(place(db[..., a:b])) for a, b in zip(CUTS[:-1], CUTS[1:])]
        assert [int(p.shape[-1]) for p in parts] == [b - a for a, b in zip(CUTS[:-1], CUTS[1:])]
        joined = torch.cat(parts, dim=-1) if where == "device" else np.concatenate(parts, axis=-1)
        same_bits(joined, whole, "the partition against one chunk")
        assert stage.flush() == []
        stage.reset()
    assert not host(whole)[:, :3].any() and host(whole)[:, 3:].all()


def test_contrast_stage_is_the_unclamped_entry():
    s = tied_plane()
    c = Stft.Config.create(fft_size=2048, hop=512)
    stage = S.spectral_contrast_stage(c, sample_rate=SR, quantile=0.04)
    whole = host(stage.step(dev(s)))
    for a, b in zip(CUTS[:-1], CUTS[1:]):
        chunk = np.ascontiguousarray(s[..., a:b])
        got = stage.step(dev(chunk))
        want = np.zeros((3, 7, b - a), np.float32)
        check(lib.smx_spectral_contrast_of_spectrogram_f32(C.c_void_p(chunk.ctypes.data), 3, 1025, b - a, 2048, 6, 200.0, 0.04, 0, SR, 0,
                                                           C.c_void_p(want.ctypes.data)))
        same_bits(got, want, "the stage against the entry")
        same_bits(got, whole[..., a:b], "the chunk against the whole")
