"""The host-array faces of FIR, Resample, Cqt and the constant-Q chroma must give the bits of the device-tensor call on the same
data.  Cqt and the constant-Q chroma go through the library's one upload / run / download path (host_call,
soundml_amd/csrc/capi.cpp); FIR and Resample keep their plain copies (profiles/host_faces/NOTES.md).

Two sizes per entry point: three channels or clips of a few thousand samples (an odd count: a wrong clip stride shows), and
one input just above the 4 MiB under which transfer.cpp copies directly, so host_call's staged copy runs.  With no clips every
entry point returns before it looks at a pointer or a device.  None of the seven has an optional input, so there is no
null-input case.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import soundml_amd as S
from soundml_amd import Chroma, Cqt, Fir, Resample
from soundml_amd._lib import check, lib
from conftest import ref_shape_digests, shape_digest
from oracle import soundml_oracle as O

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SMALL, LARGE = (3, 5001), (2, 600000)   # float32: 60 kB and 4.8 MB (the direct copy ends at 4 MiB = 4 194 304 bytes)


def dev(a):
    return torch.from_numpy(np.array(a, copy=True, order="C")).to("cuda:0")


def same(host_result, device_result):
    assert isinstance(host_result, np.ndarray) and device_result.is_cuda
    return torch.equal(torch.from_numpy(host_result), device_result.cpu())


@functools.lru_cache(maxsize=None)
def audio(shape):
    x = np.random.default_rng(shape[0] * shape[1]).uniform(-1, 1, size=shape).astype(np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def fir_plan():
    return Fir.Plan.create(Fir.design_lowpass(63, 0.25, 80.0))


@functools.lru_cache(maxsize=None)
def halving_stage():
    return Resample.Stage.create(Resample.prototype(1, 40, 0.45 / 2, O.kaiser_beta(100.0)), 1, 2, 40)


@functools.lru_cache(maxsize=None)
def direct_config():
    c = Resample.Config.create(44100, 48000)
    assert c.executor == "direct"   # (the overlap-save executor is Stage.apply's entry point)
    return c


@functools.lru_cache(maxsize=None)
def cqt_config():
    return Cqt.Config.create(36, 22050, fmin=110.0)


@pytest.mark.parametrize("shape", [SMALL, LARGE])
def test_fir_apply(shape):
    x = audio(shape)
    assert same(Fir.apply(fir_plan(), x), Fir.apply(fir_plan(), dev(x)))


@pytest.mark.parametrize("shape", [SMALL, LARGE])
def test_resample_stage_apply(shape):
    x = audio(shape)
    assert same(Resample.Stage.apply(halving_stage(), x), Resample.Stage.apply(halving_stage(), dev(x)))


@pytest.mark.parametrize("shape", [SMALL, LARGE])
def test_resample_apply(shape):
    x = audio(shape)
    assert same(Resample.apply(direct_config(), x), Resample.apply(direct_config(), dev(x)))


@pytest.mark.parametrize("shape", [SMALL, LARGE])
def test_cqt_transform_and_power_spectrum(shape):
    x = audio(shape)
    assert same(Cqt.transform(cqt_config(), x), Cqt.transform(cqt_config(), dev(x)))
    assert same(Cqt.power_spectrum(cqt_config(), x, power=1.0), Cqt.power_spectrum(cqt_config(), dev(x), power=1.0))


@pytest.mark.parametrize("shape", [(3, 36, 41), (2, 36, 16000)])   # the large one: 4.6 MB of float32
def test_chroma_of_cqt(shape):
    s = np.abs(audio((shape[0] * shape[1], shape[2]))).reshape(shape)
    for norm in ("inf", 2.0):
        assert same(Chroma.of_cqt(cqt_config(), s, norm=norm), Chroma.of_cqt(cqt_config(), dev(s), norm=norm))


@pytest.mark.parametrize("shape", [SMALL, LARGE])
def test_chroma_cqt(shape):
    x = audio(shape)
    assert same(S.chroma_cqt(cqt_config(), x), S.chroma_cqt(cqt_config(), dev(x)))


def shape_on_device(spec, oh, n, l, m):
    d_x, d_h = dev(spec), dev(oh)
    w = n * l if l > 1 else n // m
    out = torch.empty(spec.shape[:-1] + (w // 2 + 1,), dtype=torch.complex128, device="cuda:0")
    check(lib.smx_resample_shape_c128_dev(C.c_void_p(d_x.data_ptr()), C.c_void_p(d_h.data_ptr()), C.c_void_p(out.data_ptr()),
                                          spec.shape[0], n, l, m, C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    return out


def test_resample_shape():
    """The inputs of test_resample_shape_is_the_reference_stub_bit_for_bit at its smallest (l, m): the result has the digest of
    the reference's own `soundml_resample_shape_run`.  h is one array for all lines; 300 lines are 4.9 MB of complex128."""
    l, m, n, k = 1, 1, 2048, 5
    rng = np.random.default_rng(7 * l + m)
    proto = rng.uniform(-1, 1, size=2 * k * l + 1)
    oh = O.ols_plan_spectrum(proto, n, l, m)
    spec = np.fft.rfft(rng.uniform(-1, 1, size=(9, n)), axis=-1)
    want_in, want_out = ref_shape_digests("gpu", l, m)
    assert shape_digest(spec, oh) == want_in, "inputs differ from those the reference's digests were taken on"
    got = Resample.shape(spec, oh, n, l, m)
    assert shape_digest(got) == want_out
    assert same(got, shape_on_device(spec, oh, n, l, m))
    large = np.fft.rfft(rng.uniform(-1, 1, size=(300, n)), axis=-1)
    got = Resample.shape(large, oh, n, l, m)
    assert same(got, shape_on_device(large, oh, n, l, m))
    assert np.array_equal(got[299:], Resample.shape(large[299:], oh, n, l, m))   # lines are independent


def test_no_clips_is_no_device_call():
    """lead == 0 (and, for the stage and the converter, no output sample) returns before the null pointers are looked at."""
    c, (kind, p) = cqt_config(), Chroma.norm_args("inf")
    check(lib.smx_fir_apply_f32(fir_plan()._h, None, 0, 100, None))
    check(lib.smx_resample_stage_apply_f32(halving_stage()._h, None, 0, 100, None))
    check(lib.smx_resample_stage_apply_f32(halving_stage()._h, None, 3, 0, None))
    check(lib.smx_resample_apply_f32(direct_config()._h, None, 0, 100, None))
    check(lib.smx_resample_apply_f32(direct_config()._h, None, 3, 0, None))
    check(lib.smx_resample_shape_c128(None, None, None, 0, 2048, 1, 1))
    check(lib.smx_cqt_transform_f32(c._h, None, 0, 4096, None))
    check(lib.smx_cqt_power_spectrum_f32(c._h, None, 0, 4096, 2.0, None))
    check(lib.smx_chroma_of_cqt_f32(c._h, None, 0, c.n_bins, 41, 12, kind, p, None))
    check(lib.smx_chroma_cqt_f32(c._h, None, 0, 4096, 12, kind, p, None))
    assert Fir.apply(fir_plan(), np.zeros((0, 100), np.float32)).shape == (0, 100)
    assert S.chroma_cqt(c, np.zeros((0, 4096), np.float32)).shape == (0, 12, 9)
