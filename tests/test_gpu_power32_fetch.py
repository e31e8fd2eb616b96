"""The sample fetch of stft2048_power32_kernel (stft_fast_p32.hpp, load_frame32): odd waves request the upper half of their
frames' samples first, so that neighbouring waves ask the L1 for the same lines at the same step -- same registers, same
addresses, another order, behind a wave-uniform branch.  (The second change tried with it, a touch of the lines that the
workgroup's tile after next reads first, lost its A/B and is not in the code: profiles/r09/NOTES.md.  These shapes were chosen
for its address arithmetic -- the tile after next, the step into the next clip, rows with padding between the clips, a sample
pointer off the 8-byte grid, border tiles -- and they are the ones at which a fetch that depends on the wave and on the tile walk
can go wrong.)  A load into a register nobody reads cannot be observed by any test; what is checked is that every value stays
what it was: against the float64 oracle at 1e-5 of the peak, and bit for bit against the border epilogue (SMX_BORDER_INLINE=0),
whose interior launch walks other tile ranges, and against the same request walked by ONE workgroup (SMX_FAST_BLOCKS=1: clip
boundaries then fall inside the workgroup's range, and every tile but the last has a successor).  Fft 2048 / hop 512 throughout."""
import ctypes as C
import os

import numpy as np
import pytest

from soundml_amd import Stft
from soundml_amd._lib import check, lib
from oracle import soundml_oracle as O

pytestmark = pytest.mark.gpu

FFT, HOP, BINS = 2048, 512, 1025
GATE = 1e-5           # of the spectrogram's peak


def _configs(pad):
    okw = dict(hop=HOP)
    if isinstance(pad, tuple):
        okw["pad"], okw["pad_value"] = pad
    else:
        okw["pad"] = pad
    return Stft.Config.create(fft_size=FFT, hop=HOP, pad=pad), O.stft_config(FFT, **okw)


def _power(c, buf, offset, clips, n, stride, p0, p1, **env):
    """smx_stft_power_range_f32_dev on `clips` rows of n samples, `stride` floats apart, from buf[offset] on (device, flat)"""
    import torch
    out = torch.empty(clips, BINS, p1 - p0, device=buf.device, dtype=torch.float32)
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        check(lib.smx_stft_power_range_f32_dev(c._h, C.c_void_p(buf.data_ptr() + 4 * offset), C.c_int64(clips), C.c_int64(n), C.c_int64(stride),
                                               C.c_int64(p0), C.c_int64(p1), C.c_double(2.0), C.c_void_p(out.data_ptr()),
                                               C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        torch.cuda.synchronize()
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return out


def _case(clips, n, stride=None, offset=0, pad="reflect", seed=0):
    """the request as it ships, by one workgroup and through the border epilogue: equal bit for bit, and within the gate of the oracle"""
    import torch
    stride = stride or n
    rng = np.random.default_rng(1000 * clips + n + seed)
    flat = rng.uniform(-1, 1, size=offset + clips * stride).astype(np.float32)   # (the padding between the clips holds samples too: a frame that read them would differ)
    buf = torch.from_numpy(flat).cuda()
    c, o = _configs(pad)
    frames = Stft.frames(c, n)
    got = _power(c, buf, offset, clips, n, stride, 0, frames)
    assert torch.equal(got, _power(c, buf, offset, clips, n, stride, 0, frames, SMX_FAST_BLOCKS="1")), "one workgroup"
    assert torch.equal(got, _power(c, buf, offset, clips, n, stride, 0, frames, SMX_BORDER_INLINE="0")), "border epilogue"
    assert torch.equal(got, _power(c, buf, offset, clips, n, stride, 0, frames, SMX_BORDER_INLINE="0", SMX_FAST_BLOCKS="1")), "border epilogue, one workgroup"
    got = got.cpu().numpy()
    for i in range(clips):
        x = flat[offset + i * stride:offset + i * stride + n]
        want = O.power_spectrum(o, x)
        assert got[i].shape == want.shape
        assert np.max(np.abs(got[i].astype(np.float64) - want)) <= GATE * float(np.max(want)), (clips, n, stride, offset, pad, i)
    return buf, c, frames


@pytest.mark.parametrize("n", [
    FFT,                   # one tile, nothing after it
    FFT + HOP * 15,        # 20 frames
    FFT + HOP * 16,        # 21 frames: either side of a tile's sixteen
    FFT + HOP * 47,        # 52 frames, four tiles
])
def test_one_clip(n):
    _case(1, n)


N3 = FFT + HOP * 20        # 25 frames a clip, two tiles: in one workgroup's range the next tile lies in the next clip


def test_three_clips_with_padded_rows():
    """x_stride > n: the next clip's first frames are at clip + stride, and the padding behind clip + n holds other samples"""
    _case(3, N3, stride=N3 + 1000)


def test_three_clips_from_an_odd_sample_pointer():
    """the sample pointer one float off the 8-byte grid (ALIGNED = false); rows an odd number of floats apart as well"""
    _case(3, N3, stride=N3 + 1000, offset=1)
    _case(3, N3, stride=N3 + 1001, offset=1, seed=1)


@pytest.mark.parametrize("n", [FFT + HOP * 22, FFT + HOP * 21])
def test_three_clips_by_frame_count(n):
    """27 frames a clip (odd rows: the frame-per-lane flush, SKEW = 2) and 26 (even rows: a pair of frames per lane, SKEW = 1)"""
    _case(3, n, stride=n + 1000)


@pytest.mark.parametrize("pad", ["reflect", "edge", ("constant", 0.37)])
def test_three_clips_under_every_pad_mode(pad):
    _case(3, N3, stride=N3 + 1000, pad=pad, seed=2)


def test_a_range_call_is_the_slice_of_the_full_call():
    """p0 > 0 and a count that ends inside a tile, as it ships and walked by one workgroup"""
    import torch
    n = FFT + HOP * 47
    buf, c, frames = _case(3, n, stride=n + 1000, seed=3)
    full = _power(c, buf, 0, 3, n, n + 1000, 0, frames)
    for p0, p1 in ((3, 40), (1, frames - 1), (17, 17 + 16 + 5)):
        for env in ({}, {"SMX_FAST_BLOCKS": "1"}):
            assert torch.equal(_power(c, buf, 0, 3, n, n + 1000, p0, p1, **env), full[:, :, p0:p1]), (p0, p1, env)
