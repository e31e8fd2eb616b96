"""Mel.invert, mel_to_stft / mel_to_audio, mfcc_to_mel / mfcc_to_audio on the device (DESIGN.md "Mel inversion").

The yardsticks: the float64 numpy restatement of the stated algorithm (tests/inversion_restatement.py), the residuals it reaches
on consistent targets (tests/golden/inversion/residuals.json), and laws that hold bit for bit whatever the algorithm: slices,
faces, the two kernels, the compositions.  Every figure a gate compares is printed before the gate."""
import functools
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

import soundml_amd as S
from soundml_amd import Mel, Stft
from conftest import ROOT, load_golden

import inversion_restatement as R

pytestmark = pytest.mark.gpu

RECORDED = load_golden("inversion", "residuals")
# frames per clip: under one wave's width of bins / the singular Gram matrix, 201 bins on 4 x 64 slots / the long upper bands and
# a frame count that fills no whole workgroup of eight / an htk bank without the area norm
FRAMES = {"fft64_mel8": 37, "fft400_mel80": 19, "fft2048_mel128": 70, "fft512_mel40_htk": 23}
LEADS = [(3,), (2, 2)]
ROUNDS = (0, 1, 7, 200)
CLIPS = 4


def config(name):
    n_mels, sr, fft, scale, norm = R.BANKS[name]
    return Mel.Config.create(n_mels, sr, fft, scale=scale, norm=norm)


def clips_of(cols, frames):
    """[rows; CLIPS * frames] -> [CLIPS; rows; frames]"""
    return np.ascontiguousarray(cols.reshape(cols.shape[0], CLIPS, frames).transpose(1, 0, 2))


@functools.lru_cache(maxsize=None)
def case(name):
    """consistent targets m = W s for CLIPS clips, and the restatement's iterates after each count of ROUNDS: float64 and float32
    on the float32 targets, float64 on the float64 ones; computed once, read-only"""
    w = R.bank_weights(name)
    frames = FRAMES[name]
    cols = w @ R.synthetic_spectra(w.shape[1], CLIPS * frames)
    cols32 = cols.astype(np.float32)
    out = {"w": w, "m64": clips_of(cols, frames), "m32": clips_of(cols32, frames)}
    for key, src, dt in (("s64_of32", cols32.astype(np.float64), np.float64), ("s32_of32", cols32, np.float32), ("s64_of64", cols, np.float64)):
        _, snap = R.mel_invert(w, src, max(ROUNDS), dt, snapshots=ROUNDS)
        out[key] = {k: clips_of(v, frames) for k, v in snap.items()}
    for v in out.values():
        for a in (v.values() if isinstance(v, dict) else [v]):
            a.setflags(write=False)
    return out


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def host(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)


def shaped(a, lead):
    n = int(np.prod(lead))
    return a[:n].reshape(lead + a.shape[1:])


def frame_distance(got, want):
    """max_k |got - want| over the frame's largest wanted value, per (clip, frame)"""
    return np.abs(got.astype(np.float64) - want).max(axis=-2) / want.max(axis=-2)


@pytest.mark.parametrize("n_iter", ROUNDS)
@pytest.mark.parametrize("lead", LEADS, ids=str)
@pytest.mark.parametrize("name", sorted(FRAMES))
def test_float32_device(name, lead, n_iter):
    c = case(name)
    w = c["w"]
    m = shaped(c["m32"], lead)
    got = host(Mel.invert(config(name), dev(m), n_iter))
    assert got.dtype == np.float32 and got.shape == lead + (w.shape[1], FRAMES[name])
    assert (got >= 0.0).all()
    untouched = (w != 0.0).sum(axis=0) == 0
    assert untouched.any()          # DC and Nyquist: the feet of the first and the last triangle
    assert not got[..., untouched, :].any()
    if n_iter == 0:
        assert not got.any()
        return
    want64 = shaped(c["s64_of32"][n_iter], lead)
    cpu = float(frame_distance(shaped(c["s32_of32"][n_iter], lead), want64).max())
    dist = frame_distance(got, want64)
    print("\n%s lead %s n_iter %d: float32 device vs float64 restatement %.3g of the frame's maximum (numpy float32: %.3g)"
          % (name, lead, n_iter, float(dist.max()), cpu))
    assert (dist <= 4.0 * cpu).all()
    if n_iter == 200:
        flat_s = got.reshape((-1,) + got.shape[-2:])
        flat_m = m.reshape((-1,) + m.shape[-2:])
        res = np.array([R.relative_residual(w, s, t) for s, t in zip(flat_s, flat_m)])
        print("%s lead %s: relative residual after 200 rounds: max %.3g, median %.3g (float64 restatement, recorded: %.3g)"
              % (name, lead, float(res.max()), float(np.median(res)), RECORDED[name]["residual_200"]))
        assert (res <= 2.0 * RECORDED[name]["residual_200"] + 1e-5).all()


@pytest.mark.parametrize("name", sorted(FRAMES))
def test_float64_faces(name):
    c = case(name)
    cfg = config(name)
    m = shaped(c["m64"], (3,))
    for n_iter in ROUNDS:
        got = host(Mel.invert(cfg, dev(m), n_iter))
        assert got.dtype == np.float64
        want = shaped(c["s64_of64"][n_iter], (3,))
        if n_iter == 0:
            assert not got.any()
            continue
        dist = float(frame_distance(got, want).max())
        print("\n%s n_iter %d: float64 device vs restatement %.3g" % (name, n_iter, dist))
        assert dist <= 1e-9
        assert np.array_equal(got, Mel.invert(cfg, m, n_iter)), "host face != device face"


@pytest.mark.parametrize("name", sorted(FRAMES))
def test_slices_and_faces_bit_for_bit(name):
    c = case(name)
    cfg = config(name)
    m = dev(shaped(c["m32"], (2, 2)))
    frames = FRAMES[name]
    for n_iter in (7, 200):
        full = Mel.invert(cfg, m, n_iter)
        for a, b in ((3, frames - 2), (0, 1), (frames - 9, frames)):
            assert torch.equal(full[..., a:b], Mel.invert(cfg, m[..., a:b], n_iter)), (n_iter, a, b)
        assert torch.equal(full[1:], Mel.invert(cfg, m[1:], n_iter))
        assert torch.equal(full[0, 1], Mel.invert(cfg, m[0, 1], n_iter))
        on_host = Mel.invert(cfg, host(m), n_iter)
        assert isinstance(on_host, np.ndarray) and np.array_equal(on_host, host(full))


CHILD = """
import sys
import numpy as np, torch
sys.path.insert(0, %r); sys.path.insert(0, %r)
import test_gpu_mel_invert as T
out = {}
for name in sorted(T.FRAMES):
    c = T.case_inputs(name)
    for key in ("m32", "m64"):
        for n_iter in (7, 200):
            out["%%s/%%s/%%d" %% (name, key, n_iter)] = T.host(T.Mel.invert(T.config(name), T.dev(c[key]), n_iter))
np.savez(sys.argv[1], **out)
"""


def case_inputs(name):
    """the targets alone (the child of test_fast_kernel_equals_general_kernel needs no restatement)"""
    w = R.bank_weights(name)
    cols = w @ R.synthetic_spectra(w.shape[1], CLIPS * FRAMES[name])
    return {"m64": clips_of(cols, FRAMES[name]), "m32": clips_of(cols.astype(np.float32), FRAMES[name])}


def test_fast_kernel_equals_general_kernel():
    """SMX_DISABLE_FAST in a fresh process: one workgroup per frame over scratch memory instead of one wave per frame over
    registers and LDS, the same bits in both dtypes"""
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "general.npz")
        subprocess.run([sys.executable, "-c", CHILD % (ROOT, os.path.join(ROOT, "tests")), path], check=True,
                       env=dict(os.environ, SMX_DISABLE_FAST="1"), timeout=300)
        general = dict(np.load(path))
    assert len(general) == 4 * 2 * 2
    for key, want in general.items():
        name, which, n_iter = key.split("/")
        got = host(Mel.invert(config(name), dev(case_inputs(name)[which]), int(n_iter)))
        assert got.dtype == want.dtype and np.array_equal(got, want), key


@pytest.mark.parametrize("name", ["fft64_mel8", "fft2048_mel128"])
def test_mel_to_stft_is_the_root_of_invert(name):
    c = case(name)
    cfg = config(name)
    for m in (dev(shaped(c["m32"], (3,))), dev(shaped(c["m64"], (3,)))):
        s = host(Mel.invert(cfg, m, 7))
        assert np.array_equal(host(S.mel_to_stft(cfg, m, n_iter=7)), np.sqrt(s))          # power 2: a correctly rounded square root
        assert np.array_equal(host(S.mel_to_stft(cfg, m, power=1.0, n_iter=7)), s)
        got = host(S.mel_to_stft(cfg, m, power=3.0, n_iter=7))
        want = s.astype(np.float64) ** (1.0 / 3.0)
        assert (np.abs(got - want) <= np.spacing(np.abs(want).astype(s.dtype))).all()         # any other: float64 pow, one rounding
        assert np.array_equal(host(S.mel_to_stft(cfg, host(m), power=3.0, n_iter=7)), got)    # host face == device face


@pytest.mark.parametrize("name,hop", [("fft64_mel8", 16), ("fft2048_mel128", 512)])
def test_compositions_bit_for_bit(name, hop):
    c = case(name)
    cfg = config(name)
    n_mels, _, fft = R.BANKS[name][:3]
    sc = Stft.Config.create(fft_size=fft, hop=hop)
    m = dev(shaped(c["m32"], (2, 2)))
    audio = S.mel_to_audio(sc, cfg, m, n_iter=7, gl_iter=3)
    assert audio.is_cuda and audio.shape[:2] == (2, 2)
    assert torch.equal(audio, Stft.griffin_lim(sc, S.mel_to_stft(cfg, m, n_iter=7), 3))
    length = int(audio.shape[-1]) - 5
    assert torch.equal(S.mel_to_audio(sc, cfg, m, power=1.0, n_iter=7, gl_iter=2, momentum=0.5, length=length),
                       Stft.griffin_lim(sc, S.mel_to_stft(cfg, m, 1.0, 7), 2, 0.5, None, length))
    rng = np.random.default_rng(11)
    cep = dev((rng.normal(size=(2, min(13, n_mels), FRAMES[name])) * 4.0).astype(np.float32))
    got = S.mfcc_to_audio(sc, cfg, cep, lifter=22.0, reference=0.5, n_iter=7, gl_iter=2)
    assert torch.equal(got, S.mel_to_audio(sc, cfg, S.mfcc_to_mel(cep, n_mels, 22.0, 0.5), n_iter=7, gl_iter=2))


@pytest.mark.parametrize("n_mfcc,n_mels,lifter,reference", [(13, 40, 22.0, 1.0), (40, 40, None, 2.5), (1, 1, None, 1.0), (33, 128, 0.0, 1.0)])
def test_mfcc_to_mel_against_the_restatement(n_mfcc, n_mels, lifter, reference):
    rng = np.random.default_rng(n_mfcc)
    c64 = rng.normal(size=(2, 3, n_mfcc, 67)) * 6.0
    for dtype in (np.float32, np.float64):
        c = c64.astype(dtype)
        want = R.mfcc_to_mel(c, n_mels, lifter, reference)
        got = host(S.mfcc_to_mel(dev(c), n_mels, lifter, reference))
        assert got.dtype == dtype and got.shape == (2, 3, n_mels, 67)
        err = np.abs(got.astype(np.float64) - want)
        if dtype == np.float32:
            assert (err <= np.spacing(want.astype(np.float32)).astype(np.float64) + 1e-11).all(), float((err / want).max())
        else:
            assert (err <= 1e-9 * want).all(), float((err / want).max())
        assert np.array_equal(S.mfcc_to_mel(c, n_mels, lifter, reference), got)      # host face == device face
        assert torch.equal(S.mfcc_to_mel(dev(c)[1:, :, :, 5:40], n_mels, lifter, reference), dev(got)[1:, :, :, 5:40])


def test_empty_results():
    cfg = config("fft64_mel8")
    for dt in (torch.float32, torch.float64):
        assert tuple(Mel.invert(cfg, torch.zeros(3, 8, 0, dtype=dt, device="cuda:0")).shape) == (3, 33, 0)
        assert tuple(Mel.invert(cfg, torch.zeros(0, 2, 8, 5, dtype=dt, device="cuda:0")).shape) == (0, 2, 33, 5)
        assert tuple(S.mfcc_to_mel(torch.zeros(0, 13, 5, dtype=dt, device="cuda:0"), 20).shape) == (0, 20, 5)
    assert Mel.invert(cfg, np.zeros((8, 0), np.float32)).shape == (33, 0)
    assert S.mel_to_stft(cfg, np.zeros((2, 8, 0))).shape == (2, 33, 0)


def message(call):
    with pytest.raises(S.InvalidArgument) as e:
        call()
    return str(e.value)


def test_error_paths():
    cfg = config("fft64_mel8")
    m = torch.ones(2, 8, 5, device="cuda:0")
    assert message(lambda: Mel.invert(cfg, m[0, 0])) == \
        "invert: cannot invert a rank-1 tensor (the mel inversion needs [...; n_mels; frames])"
    assert message(lambda: Mel.invert(cfg, m[:, :7])) == \
        "invert: cannot invert 7 mel bands through a filterbank of 8 filters (the mel axis must hold n_mels values)"
    assert message(lambda: Mel.invert(cfg, m, n_iter=-1)) == "invert: cannot run -1 iterations (n_iter must be non-negative)"
    plain = Mel.Config.from_weights(Mel.filterbank(np.float64, cfg), 64)
    for arg in (m, m.cpu().numpy(), m.double()):
        assert message(lambda: Mel.invert(plain, arg)).startswith(
            "invert: cannot invert through a filterbank built from caller-supplied weights")
    for power in (0.0, -2.0, float("inf"), float("nan")):
        assert "power must be finite and positive" in message(lambda: S.mel_to_stft(cfg, m, power=power))
    sc = Stft.Config.create(fft_size=128, hop=32)
    for fn, call in (("mel_to_audio", lambda: S.mel_to_audio(sc, cfg, m)), ("mfcc_to_audio", lambda: S.mfcc_to_audio(sc, cfg, m))):
        assert message(call) == ("%s: cannot project a 128-point STFT through a filterbank built for an FFT of size 64 (the two "
                                 "configurations must agree on fft_size)" % fn)
    c = torch.ones(2, 13, 5, device="cuda:0")
    assert "n_mels must be at least n_mfcc" in message(lambda: S.mfcc_to_mel(c, 12))
    assert message(lambda: S.mfcc_to_mel(c[0, 0], 20)) == \
        "mfcc_to_mel: cannot invert a rank-1 tensor (the cepstral and frame axes must exist)"
    for lifter in (-1.0, float("inf"), float("nan")):
        assert "lifter must be finite and non-negative" in message(lambda: S.mfcc_to_mel(c, 20, lifter=lifter))
    # 1 + (2 / 2) sin (3 pi / 2) is exactly zero: coefficient 2 cannot be un-liftered
    assert message(lambda: S.mfcc_to_mel(c, 20, lifter=2.0)) == \
        "mfcc_to_mel: cannot undo a lifter of 2 (its weight for coefficient 2 is zero)"
    assert S.mfcc_to_mel(c[:, :2], 20, lifter=2.0).shape == (2, 20, 5)
    assert message(lambda: S.mfcc_to_mel(c, 20, reference=0.0)) == "Soundml.Convert.db_to_power: reference must be finite and positive"
    # the solver of a Griffin-Lim inversion is checked before any work: the synthesis checks are griffin_lim's own
    assert "griffin_lim" in message(lambda: S.mel_to_audio(Stft.Config.create(fft_size=64, hop=16), cfg, m, gl_iter=0))
