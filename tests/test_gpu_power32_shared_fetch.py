"""The shared sample fetch of stft2048_power32_kernel (stft_fast_p32.hpp, load_pair32_shared / unpack_pair32): a wave whose two
halves hold consecutive frames fetches the 2560 samples they span once, 20 requests of 512 contiguous bytes, and deals them out
to the halves by v_permlane32_swap -- the same sample in the same register of the same lane as the 32 requests per half leave
there.  The launcher takes that kernel for an even number of frames from 8-byte aligned samples (SMX_P32_SHARE=0: never), so the
shapes below sit on both sides of every condition, and of every exception inside a tile: border waves beside shared ones, waves
without frames, clips that begin inside a workgroup's walk.  Every value must stay what it was: within 1e-5 of the peak of the
float64 oracle, and bit for bit equal to the same call with the requests per half, walked by one workgroup, and through the border
epilogue.  The samples around and between the clips are random too: a frame that read them would differ.  Fft 2048 / hop 512."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from soundml_amd import Stft
from soundml_amd._lib import check, lib
from oracle import soundml_oracle as O

pytestmark = pytest.mark.gpu

FFT, HOP, BINS = 2048, 512, 1025
GATE = 1e-5           # of the spectrogram's peak
N48 = HOP * 47        # 48 frames, three tiles: shared-span waves between the border waves of the first and the last tile
N49 = HOP * 48        # 49 frames: the last tile holds one frame (the launcher keeps the requests per half)
TAIL = 777            # samples behind the last clip


def _configs(pad):
    okw = dict(hop=HOP)
    if isinstance(pad, tuple):
        okw["pad"], okw["pad_value"] = pad
    else:
        okw["pad"] = pad
    return Stft.Config.create(fft_size=FFT, hop=HOP, pad=pad), O.stft_config(FFT, **okw)


def _power(c, buf, offset, clips, n, stride, p0, p1, power=2.0, **env):
    """smx_stft_power_range_f32_dev on `clips` rows of n samples, `stride` floats apart, from buf[offset] on (device, flat)"""
    import torch
    out = torch.empty(clips, BINS, p1 - p0, device=buf.device, dtype=torch.float32)
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        check(lib.smx_stft_power_range_f32_dev(c._h, C.c_void_p(buf.data_ptr() + 4 * offset), C.c_int64(clips), C.c_int64(n), C.c_int64(stride),
                                               C.c_int64(p0), C.c_int64(p1), C.c_double(power), C.c_void_p(out.data_ptr()),
                                               C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        torch.cuda.synchronize()
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return out


@functools.lru_cache(maxsize=None)
def _signal(clips, n, stride, offset, seed):
    rng = np.random.default_rng(1000 * clips + n + 7 * stride + offset + seed)
    flat = rng.uniform(-1, 1, size=offset + clips * stride + TAIL).astype(np.float32)
    flat.setflags(write=False)
    return flat


@functools.lru_cache(maxsize=None)
def _oracle(clips, n, stride, offset, seed, pad, power):
    """float64 reference of every clip, computed once per signal and shared (read-only)"""
    flat = _signal(clips, n, stride, offset, seed)
    o = _configs(pad)[1]
    want = np.stack([O.power_spectrum(o, flat[offset + i * stride:offset + i * stride + n].astype(np.float64), power) for i in range(clips)])
    want.setflags(write=False)
    return want


def _case(clips, n, stride=None, offset=0, pad="reflect", seed=0, power=2.0, ranges=(None,), blocks=("1",)):
    import torch
    stride = stride or n
    flat = _signal(clips, n, stride, offset, seed)
    want_full = _oracle(clips, n, stride, offset, seed, pad, power)
    buf = torch.tensor(flat, device="cuda")
    c = _configs(pad)[0]
    frames = Stft.frames(c, n)
    assert want_full.shape == (clips, BINS, frames)
    for r in ranges:
        p0, p1 = r or (0, frames)
        call = functools.partial(_power, c, buf, offset, clips, n, stride, p0, p1, power)
        got = call()
        want = want_full[:, :, p0:p1]
        err = np.max(np.abs(got.cpu().numpy().astype(np.float64) - want), axis=(1, 2))
        peak = np.max(want, axis=(1, 2))
        print("clips %d n %d stride %d offset %d pad %s power %g frames [%d, %d): max error / peak %.3g" % (clips, n, stride, offset, pad, power, p0, p1, float(np.max(err / peak))))
        assert np.all(err <= GATE * peak), (clips, n, stride, offset, pad, power, r)
        assert torch.equal(got, call(SMX_P32_SHARE="0")), ("requests per half", r)
        assert torch.equal(got, call(SMX_BORDER_INLINE="0")), ("border epilogue", r)
        for b in blocks:
            assert torch.equal(got, call(SMX_FAST_BLOCKS=b)), ("workgroups", b, r)
            assert torch.equal(got, call(SMX_FAST_BLOCKS=b, SMX_P32_SHARE="0")), ("workgroups, requests per half", b, r)


def test_interior_pairs_beside_border_waves():
    """48 frames: the pair-form flush; wave 0 of the first tile and the waves behind frame 45 take the padding rule"""
    _case(3, N48)


def test_odd_frame_count():
    """49 frames: the last tile has a wave with one frame and waves with none; the frame-per-lane flush"""
    _case(3, N49)


@pytest.mark.parametrize("n", [480000 // 16, 5120 + 2048])
def test_tail_short_of_a_tile(n):
    """59 frames (a tail of 11) and 15 frames (one short tile)"""
    _case(2, n)


def test_clip_shorter_than_a_span():
    """n < fft + hop: an even range keeps the requests per half (a border wave's unused request reads the clip's first fft samples only)"""
    _case(2, FFT + 100, ranges=((0, 4), (1, 5), None))


def test_even_count_with_waves_without_frames():
    """a wave without frames reads its tile's first two.  18 frames: the second tile holds frames 16 and 17, both past the signal's
    end, so waves 1..7 take the padding rule on frame 16; 22 frames: 16 and 17 are interior (the span is fetched), 20 and 21 are
    not; 38 interior frames from a range of a longer clip: no border tile at all"""
    _case(2, HOP * 17)
    _case(2, HOP * 21)
    _case(2, HOP * 60, ranges=((10, 48),), seed=1)


def test_sample_pointer_offsets():
    """2 floats: 8-byte aligned and off the 512-byte grid, the shared span; 1 float: unaligned, the requests per half"""
    _case(3, N48, offset=2)
    _case(3, N48, offset=1)


def test_row_strides():
    """rows n + 6 floats apart; n + 1: every other clip is off the 8-byte grid, so the whole request is"""
    _case(3, N48, stride=N48 + 6)
    _case(3, N48, stride=N48 + 1)


def test_frame_ranges():
    """the tile origin is not the clip's frame 0: a wave's halves are frames (p0 + 2 w, p0 + 2 w + 1); an odd count last"""
    _case(3, N48, stride=N48 + 6, seed=2, ranges=((1, 47), (2, 48), (3, 37), (1, 48)))


@pytest.mark.parametrize("pad", ["edge", ("constant", 0.37)])
def test_pad_modes(pad):
    """(reflect: every other test)"""
    _case(3, N48, pad=pad, seed=3)


def test_power_one():
    """|X|: another instantiation"""
    _case(3, N48, power=1.0)
    _case(3, N49, power=1.0)


def test_a_walk_across_clips():
    """two workgroups over five clips of three tiles: the tile requested behind slot 5 belongs to the next clip"""
    _case(5, N48, stride=N48 + 6, seed=4, blocks=("1", "2"))
