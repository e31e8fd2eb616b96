"""Hpss on the device (soundml_amd/csrc/hpss.hip) against the reference's goldens and against the numpy restatement
of hpss.ml (tests/hpss_restatement.py, itself pinned to the goldens by tests/test_hpss_restatement.py).

A median selects, so the spectrogram-domain faces are compared bit for bit: hard masks by exact agreement with no
cell left out, p = 1 and p = 2 within 1 ulp of the float32 restatement (division and multiplication are correctly
rounded on both sides), a general power against numpy's powf at rtol 1e-6.  The 31 x 31 tile kernel and the
general kernel must give identical bits."""
import os

import numpy as np
import pytest

import soundml_amd as S
from soundml_amd import Hpss, Stft
from conftest import F32_ATOL, F32_RTOL, F64_ATOL, F64_RTOL, check_close
from oracle import soundml_oracle as O

import hpss_restatement as R

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
INF = float("inf")


@pytest.fixture(autouse=True)
def _default_interior():
    S.set_interior("float32")
    yield
    S.set_interior("float32")
    os.environ.pop("SMX_DISABLE_FAST", None)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def host(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)


def general(face, *args, **kw):
    """The same call on the general kernel (SMX_DISABLE_FAST: the library's switch between two implementations of one
    contract)."""
    os.environ["SMX_DISABLE_FAST"] = "1"
    try:
        return face(*args, **kw)
    finally:
        os.environ.pop("SMX_DISABLE_FAST", None)


def ulp_distance(a, e):
    """Distance in float32 units in the last place (ordered-integer difference); -0.0 == +0.0."""
    def ordered(x):
        i = np.ascontiguousarray(x, dtype=np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(ordered(a) - ordered(e))


# ---- 1. goldens, spectrogram domain ---------------------------------------------------------------------------------------
def run_golden(case, face, masks, on_device):
    p = case["params"]
    s = R.golden_spectrogram(p).astype(p["dtype"])
    pair = face(dev(s) if on_device else s, **R.golden_arguments(p))
    got = host(R.component(p, pair))
    assert got.dtype == np.dtype(p["dtype"]) and list(got.shape) == case["shape"]
    if masks and p["power"] == "inf":
        flipped = int((got.astype(np.float64).reshape(-1) != np.asarray(case["values"])).sum())
        assert flipped == 0, "%s: %d of %d cells flipped" % (case["name"], flipped, got.size)
    else:
        rtol, atol = (F64_RTOL, F64_ATOL) if p["dtype"] == "float64" else (F32_RTOL, F32_ATOL)
        check_close(got, case["values"], shape=case["shape"], rtol=rtol, atol=atol, msg=case["name"])


def device_legs(case):
    return (False, True) if case["params"]["dtype"] == "float32" else (False,)


@pytest.mark.parametrize("case", R.golden_cases("hpss"))
def test_spectrogram_goldens(case):
    for on_device in device_legs(case):
        run_golden(case, Hpss.hpss_of_spectrogram, False, on_device)


@pytest.mark.parametrize("case", R.golden_cases("hpss_boundary"))
def test_boundary_goldens(case):
    for on_device in device_legs(case):
        run_golden(case, Hpss.hpss_of_spectrogram, False, on_device)


@pytest.mark.parametrize("case", R.golden_cases("hpss_masks"))
def test_mask_goldens(case):
    for on_device in device_legs(case):
        run_golden(case, Hpss.hpss_masks, True, on_device)


# ---- 2. bit-equality with the restatement at size -----------------------------------------------------------------------------
def plane_stack(shape, seed):
    """Non-negative float32 planes with ridges, columns, a silent band and exact repeats (ties)."""
    rng = np.random.default_rng(seed)
    s = rng.random(shape, dtype=np.float32)
    s[..., 3::7, :] += np.float32(3.0)
    s[..., :, 2::5] += np.float32(2.0)
    s[..., -5:, :] = 0.0
    s[..., 40:60, 10:30] = np.float32(0.25)
    return s


KERNELS = [(31, 31), (17, 31), (32, 32), (3, 5), (64, 7)]
MARGINS = [(1.0, 1.0), (1.0, 3.0)]


@pytest.mark.parametrize("shape", [(3, 1025, 938), (2, 513, 40)], ids=["1025x938", "513x40"])
@pytest.mark.parametrize("kernel", KERNELS, ids=lambda k: "k%dx%d" % k)
def test_bit_equality_with_the_restatement(shape, kernel):
    s = plane_stack(shape, 11)
    harm, perc = R.medians(s, kernel)
    d = dev(s)
    for margin in MARGINS:
        m_h, m_p = np.float32(margin[0]), np.float32(margin[1])
        split = margin == (1.0, 1.0)
        # hard masks: exact 0 / 1, no flipped cell
        got_h, got_p = (host(t) for t in Hpss.hpss_masks(d, kernel_size=kernel, power=INF, margin=margin))
        want_h, want_p = R.softmask(harm, perc * m_h, INF, split), R.softmask(perc, harm * m_p, INF, split)
        flips = int((got_h != want_h).sum() + (got_p != want_p).sum())
        print("kernel %s margin %s power inf: %d flipped cells of %d" % (kernel, margin, flips, 2 * s.size))
        assert flips == 0
        for power in (1.0, 2.0, 1.5):
            got_h, got_p = (host(t) for t in Hpss.hpss_of_spectrogram(d, kernel_size=kernel, power=power, margin=margin))
            want_h = s * R.softmask(harm, perc * m_h, power, split)
            want_p = s * R.softmask(perc, harm * m_p, power, split)
            if power == 1.5:
                err = max(float(np.max(np.abs(got_h - want_h) - 1e-6 * np.abs(want_h))),
                          float(np.max(np.abs(got_p - want_p) - 1e-6 * np.abs(want_p))))
                print("kernel %s margin %s power 1.5: max (|a - e| - 1e-6 |e|) = %.3g" % (kernel, margin, err))
                assert err <= 0.0
            else:
                worst = int(max(ulp_distance(got_h, want_h).max(), ulp_distance(got_p, want_p).max()))
                print("kernel %s margin %s power %g: worst distance %d ulp" % (kernel, margin, power, worst))
                assert worst <= 1


@pytest.mark.parametrize("power", [INF, 1.0, 2.0, 1.5])
@pytest.mark.parametrize("margin", MARGINS)
def test_tile_kernel_and_general_kernel_give_identical_bits(power, margin):
    d = dev(plane_stack((3, 1025, 938), 12))
    for face in (Hpss.hpss_masks, Hpss.hpss_of_spectrogram):
        fast = face(d, power=power, margin=margin)
        slow = general(face, d, power=power, margin=margin)
        for a, b in zip(fast, slow):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))


# ---- 3. the complex face ---------------------------------------------------------------------------------------------------------
def noise_spectrum():
    rng = np.random.default_rng(7)
    x = (rng.random((4, 96000), dtype=np.float32) * 2 - 1).astype(np.float32)
    c = Stft.Config.create(fft_size=2048, hop=512)
    z = Stft.transform(c, x)
    assert z.dtype == np.complex64 and z.shape == (4, 1025, Stft.frames(c, 96000))   # (188 frames with the default centred, reflect-padded grid)
    return c, x, z


@pytest.mark.parametrize("kernel,margin", [((31, 31), (1.0, 1.0)), ((17, 31), (1.0, 3.0)), ((32, 32), (2.0, 1.0))])
def test_complex_face_against_the_restatement(kernel, margin):
    _, _, z = noise_spectrum()
    for power in (2.0, 1.0):
        want = R.hpss_of_stft(z, kernel, power, margin)
        for container in (z, dev(z)):
            got = [host(t) for t in Hpss.hpss_of_stft(container, kernel_size=kernel, power=power, margin=margin)]
            for a, e in zip(got, want):
                assert a.dtype == np.complex64
                peak = float(np.max(np.abs(e)))
                excess = float(np.max(np.abs(a - e) - (1e-6 * np.abs(e) + 1e-7 * peak)))
                print("kernel %s margin %s power %g: max excess over the tolerance %.3g (peak %.3g)" % (kernel, margin, power, excess, peak))
                assert excess <= 0.0
    # hard masks: every output cell is 0 or z.  The only rounding ahead of the decision is |z|, so a cell may be left out only
    # if, in the restatement, 0 < |x - r| <= 4 ulp; that share is bounded on the restatement alone
    mag, harm, perc, want_h, want_p = R.of_stft_parts(z, kernel, INF, margin)
    m_h, m_p = np.float32(margin[0]), np.float32(margin[1])

    def undecided(x, r):
        gap = np.abs(x - r)
        return (gap > 0) & (gap <= 4 * np.spacing(np.maximum(x, r)))
    skip_h, skip_p = undecided(harm, perc * m_h), undecided(perc, harm * m_p)
    share = (int(skip_h.sum()) + int(skip_p.sum())) / (2.0 * mag.size)
    ties = float((harm == perc).mean())
    print("kernel %s margin %s: %d + %d undecided cells of %d, exact ties %.4f" % (kernel, margin, int(skip_h.sum()), int(skip_p.sum()), mag.size, ties))
    assert share <= 1e-4
    for container in (z, dev(z)):
        got_h, got_p = (host(t) for t in Hpss.hpss_of_stft(container, kernel_size=kernel, power=INF, margin=margin))
        for got, want, skip in ((got_h, want_h, skip_h), (got_p, want_p, skip_p)):
            keep_got, keep_want = got != 0, want != 0
            wrong = (keep_got != keep_want) & ~skip & (z != 0)
            assert int(wrong.sum()) == 0, "%d decisions differ" % int(wrong.sum())
            kept = keep_got & keep_want
            peak = float(np.max(np.abs(z)))
            assert float(np.max(np.abs(got[kept] - z[kept]), initial=0.0)) <= 1e-6 * peak


# ---- 4. the signal face ------------------------------------------------------------------------------------------------------------
def effects_face(c, x, p):
    args = R.golden_arguments(p)
    if p["face"] == "hpss":
        return R.component(p, Hpss.hpss(c, x, **args))
    return getattr(Hpss, p["face"])(c, x, **args)


@pytest.mark.parametrize("case", R.golden_cases("hpss_effects"))
def test_effects_goldens(case):
    from test_gpu_parity import check_fast
    p = case["params"]
    c = Stft.Config.create(fft_size=p["fft_size"], hop=p["hop"], pad=("constant", 0.0))
    x = O.lcg_signal(p["length"], p["seed"]).astype(p["dtype"])
    if p["dtype"] == "float64":
        got = effects_face(c, x, p)
        assert got.dtype == np.float64
        check_close(got, case["values"], shape=case["shape"], rtol=F64_RTOL, atol=F64_ATOL, msg=case["name"])
        return
    S.set_interior("float64")
    try:
        got = effects_face(c, x, p)
        assert got.dtype == np.float32
        check_close(got, case["values"], shape=case["shape"], rtol=F32_RTOL, atol=F32_ATOL, msg=case["name"] + "/strict")
    finally:
        S.set_interior("float32")
    check_fast(effects_face(c, x, p), np.asarray(case["values"]).reshape(case["shape"]), case["name"] + "/fast")
    check_fast(host(effects_face(c, dev(x), p)), np.asarray(case["values"]).reshape(case["shape"]), case["name"] + "/fast/device")


@pytest.mark.parametrize("power", [2.0, 1.0, 1.5, INF])
def test_composition_law(power):
    """Hpss.hpss is bit for bit Stft.invert of each half of Hpss.hpss_of_stft of Stft.transform; harmonic / percussive are its halves."""
    rng = np.random.default_rng(5)
    x = (rng.random((5, 30000), dtype=np.float32) * 2 - 1).astype(np.float32)
    n = x.shape[-1]
    c = Stft.Config.create(fft_size=2048, hop=512)
    kw = dict(power=power, margin=(1.0, 2.0))
    for container in (x, dev(x)):
        y_h, y_p = Hpss.hpss(c, container, **kw)
        z_h, z_p = Hpss.hpss_of_stft(Stft.transform(c, container), **kw)
        w_h, w_p = Stft.invert(c, z_h, length=n), Stft.invert(c, z_p, length=n)
        assert y_h.shape == tuple(x.shape) and y_h.dtype == container.dtype
        for got, want in ((y_h, w_h), (y_p, w_p), (Hpss.harmonic(c, container, **kw), w_h), (Hpss.percussive(c, container, **kw), w_p)):
            assert np.array_equal(host(got).view(np.int32), host(want).view(np.int32))
    x64 = x[:2, :6000].astype(np.float64)
    y_h, y_p = Hpss.hpss(c, x64, **kw)
    z_h, z_p = Hpss.hpss_of_stft(Stft.transform(c, x64), **kw)
    assert y_h.dtype == np.float64 and z_h.dtype == np.complex128
    assert np.array_equal(y_h, Stft.invert(c, z_h, length=6000)) and np.array_equal(y_p, Stft.invert(c, z_p, length=6000))


def test_signal_face_against_the_oracle():
    """Finite power at fft 2048 / hop 512, [4; 96000]: the project's bar, |a - e| <= 1e-5 peak + 1e-5 |e|."""
    from test_gpu_parity import check_fast
    c, x, _ = noise_spectrum()
    o = O.stft_config(2048, hop=512)
    for power, margin in ((2.0, (1.0, 1.0)), (1.0, (1.0, 3.0))):
        want = R.hpss(o, x, (31, 31), power, margin)
        for container in (x, dev(x)):
            got = Hpss.hpss(c, container, power=power, margin=margin)
            for a, e, name in zip(got, want, ("harmonic", "percussive")):
                check_fast(host(a), e, "%s power %g" % (name, power))


# ---- 5. laws -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", [(31, 31), (5, 64)], ids=lambda k: "k%dx%d" % k)
def test_a_batch_equals_its_slices(kernel):
    s = plane_stack((3, 300, 260), 3)
    z = (s * np.exp(1j * np.random.default_rng(4).random(s.shape) * 6.0)).astype(np.complex64)
    for face, data in ((Hpss.hpss_masks, s), (Hpss.hpss_of_spectrogram, s), (Hpss.hpss_of_stft, z)):
        for power in (2.0, 1.5, INF):
            for container in (data, dev(data)):
                whole = [host(t) for t in face(container, kernel_size=kernel, power=power, margin=(1.0, 2.0))]
                for i in range(data.shape[0]):
                    part = [host(t) for t in face(container[i], kernel_size=kernel, power=power, margin=(1.0, 2.0))]
                    for w, q in zip(whole, part):
                        assert w[i].tobytes() == q.tobytes()


def test_masks_partition_at_unit_margins():
    s = plane_stack((2, 400, 300), 8)
    harm, perc = R.medians(s, (31, 31))
    normal = np.maximum(harm, perc) >= np.finfo(np.float32).tiny
    for power in (1.0, 2.0, 1.5):
        mask_h, mask_p = (host(t) for t in Hpss.hpss_masks(dev(s), power=power))
        total = mask_h + mask_p
        assert int(ulp_distance(total[normal], np.ones_like(total[normal])).max()) <= 1
        assert np.all(mask_h[~normal] == 0.5) and np.all(mask_p[~normal] == 0.5)   # (the silent band: the partition is split)
    for margin in ((2.0, 1.0), (1.5, 3.0)):
        for power in (1.0, 2.0, INF):
            h, p = (host(t) for t in Hpss.hpss_of_spectrogram(dev(s), power=power, margin=margin))
            assert np.all(h + p <= s)


def test_device_list_equals_the_single_device_call():
    s = plane_stack((5, 200, 180), 9)
    x = (np.random.default_rng(2).random((5, 20000), dtype=np.float32) * 2 - 1).astype(np.float32)
    c = Stft.Config.create(fft_size=2048, hop=512)
    one = [Hpss.hpss_of_spectrogram(s), Hpss.hpss_masks(s, kernel_size=(7, 9), power=INF), Hpss.hpss(c, x)]
    S.set_devices([0, 0])
    try:
        two = [Hpss.hpss_of_spectrogram(s), Hpss.hpss_masks(s, kernel_size=(7, 9), power=INF), Hpss.hpss(c, x)]
    finally:
        S.set_devices([])
    for a, b in zip(one, two):
        for u, v in zip(a, b):
            assert u.tobytes() == v.tobytes()


def test_zero_size_axes():
    for shape in ((0, 9, 9), (2, 0, 9), (2, 9, 0)):
        for container in (np.zeros(shape, np.float32), dev(np.zeros(shape, np.float32)), np.zeros(shape, np.float64)):
            for face in (Hpss.hpss_masks, Hpss.hpss_of_spectrogram):
                a, b = face(container)
                assert tuple(a.shape) == shape and tuple(b.shape) == shape and a.dtype == container.dtype
        z_h, z_p = Hpss.hpss_of_stft(np.zeros(shape, np.complex64))
        assert z_h.shape == shape and z_p.dtype == np.complex64
    c = Stft.Config.create(fft_size=512, hop=128)
    for container in (np.zeros((0, 4000), np.float32), np.zeros((3, 0), np.float32), dev(np.zeros((0, 4000), np.float32))):
        y_h, y_p = Hpss.hpss(c, container)
        assert tuple(y_h.shape) == tuple(container.shape) and tuple(y_p.shape) == tuple(container.shape)


def test_validation_messages_with_device_tensors():
    """Every message of every face is checked verbatim without a device in tests/test_hpss_host.py; here the same checks come
    first when the data is on the device, and from the device entry points of the C ABI themselves."""
    import ctypes as C
    from soundml_amd._lib import lib
    s = dev(np.ones((4, 4), np.float32))
    c = Stft.Config.create(fft_size=512, hop=128)
    for fn, call in (("hpss_masks", lambda **kw: Hpss.hpss_masks(s, **kw)),
                     ("hpss_of_stft", lambda **kw: Hpss.hpss_of_stft(s.to(torch.complex64), **kw)),
                     ("percussive", lambda **kw: Hpss.percussive(c, dev(np.zeros(4000, np.float32)), **kw))):
        for kw, message in [
                (dict(kernel_size=(3, -2), power=-1.0), "cannot median-filter with a kernel of (3, -2) (both kernel sizes must be at least 1)"),
                (dict(power=0.0, margin=(0.0, 1.0)), "cannot raise the mask to the power 0 (power must be strictly positive, or infinite for a hard mask)"),
                (dict(margin=(INF, 1.0)), "cannot bias the decision by a margin of (inf, 1) (both margins must be finite and at least 1)")]:
            with pytest.raises(S.InvalidArgument) as e:
                call(**kw)
            assert str(e.value) == "%s: %s" % (fn, message)
    ptr = C.c_void_p(s.data_ptr())
    assert lib.smx_hpss_masks_f32_dev(ptr, 1, 4, 4, 0, 31, 2.0, 1.0, 1.0, ptr, ptr, None) == 1
    assert lib.smx_last_error().decode() == "hpss_masks: cannot median-filter with a kernel of (0, 31) (both kernel sizes must be at least 1)"
    assert lib.smx_hpss_f32_dev(c._h, ptr, 1, 16, 31, 31, -2.0, 1.0, 1.0, ptr, None, None) == 1
    assert lib.smx_last_error().decode() == "harmonic: cannot raise the mask to the power -2 (power must be strictly positive, or infinite for a hard mask)"
