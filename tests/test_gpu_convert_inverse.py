"""Convert.db_to_power / db_to_amplitude (convert.ml:58-68) on the host and device faces: the round trips of the reference's
test/db/test_props.ml with its tolerances, the float64 evaluation with one rounding, face against face bit for bit."""
import ctypes as C

import numpy as np
import pytest
import torch

import soundml_amd as S
from soundml_amd import Convert
from soundml_amd._lib import check, lib

pytestmark = pytest.mark.gpu

PAIRS = {
    # inverse -> (forward, gain, [lo, hi] of the log-uniform values, references)
    "db_to_power": (Convert.power_to_db, 10.0, (1e-6, 1e3), (1.0, 2.5)),
    "db_to_amplitude": (Convert.amplitude_to_db, 20.0, (1e-4, 1e2), (1.0, 0.5)),
}


def values(lo, hi, dtype):
    return np.exp(np.linspace(np.log(lo), np.log(hi), 128)).astype(dtype)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


@pytest.mark.parametrize("fn", sorted(PAIRS))
def test_round_trips(fn):
    forward, _, (lo, hi), references = PAIRS[fn]
    inverse = getattr(Convert, fn)
    for reference in references:
        v = values(lo, hi, np.float64)
        back = inverse(forward(v, reference=reference), reference=reference)
        assert back.dtype == np.float64
        np.testing.assert_allclose(back, v, rtol=1e-12, atol=1e-12)
        v = values(lo, hi, np.float32)
        back = inverse(forward(v, reference=reference), reference=reference)
        assert back.dtype == np.float32
        np.testing.assert_allclose(back, v, rtol=1e-5, atol=1e-6)
        back = inverse(forward(dev(v), reference=reference), reference=reference)
        assert back.is_cuda and back.dtype == torch.float32
        np.testing.assert_allclose(back.cpu().numpy(), v, rtol=1e-5, atol=1e-6)
        back = inverse(forward(v.astype(np.float64), reference=reference), reference=reference)   # (float64 on the device face)
        on_device = inverse(dev(forward(v.astype(np.float64), reference=reference)), reference=reference)
        assert on_device.dtype == torch.float64 and np.array_equal(on_device.cpu().numpy(), back)


@pytest.mark.parametrize("fn", sorted(PAIRS))
@pytest.mark.parametrize("reference", [1.0, 2.5, 1e-3])
def test_one_rounding_and_equal_faces(fn, reference):
    gain = PAIRS[fn][1]
    rng = np.random.default_rng(7)
    db = rng.uniform(-120.0, 60.0, size=(3, 5, 41)).astype(np.float32)
    want = reference * 10.0 ** (db.astype(np.float64) / gain)
    on_host = getattr(Convert, fn)(db, reference=reference)
    assert on_host.shape == db.shape and on_host.dtype == np.float32
    assert (np.abs(on_host.astype(np.float64) - want) <= np.spacing(want.astype(np.float32))).all()     # within one float32 ulp
    d = dev(db)
    on_device = getattr(Convert, fn)(d, reference=reference)
    assert np.array_equal(on_device.cpu().numpy(), on_host)
    # in place through the C ABI: out may alias the input
    check(getattr(lib, "smx_%s_f32_dev" % fn)(C.c_void_p(d.data_ptr()), d.numel(), reference, C.c_void_p(d.data_ptr()),
                                              C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    assert torch.equal(d, on_device)
    assert getattr(Convert, fn)(np.float32(-20.0), reference=reference).shape == ()      # a rank-zero tensor is a tensor


@pytest.mark.parametrize("fn", sorted(PAIRS))
def test_empty_and_errors(fn):
    inverse = getattr(Convert, fn)
    for empty in (np.zeros((0, 4), np.float32), np.zeros((2, 0), np.float64), torch.zeros(3, 0, device="cuda:0")):
        got = inverse(empty)
        assert type(got) is type(empty) and tuple(got.shape) == tuple(empty.shape) and got.dtype == empty.dtype
    for arg in (np.zeros(3, np.float32), torch.zeros(3, device="cuda:0"), torch.zeros(0, device="cuda:0")):
        for reference in (0.0, -2.0, float("inf"), float("nan")):
            with pytest.raises(S.InvalidArgument) as e:
                inverse(arg, reference=reference)
            assert str(e.value) == "Soundml.Convert.%s: reference must be finite and positive" % fn
