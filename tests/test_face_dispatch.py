"""``Batch.run`` and ``FramedStage`` on their own: stand-in entries that record their arguments, no device, no library call."""
import numpy as np
import pytest
import torch

from soundml_amd import _lib
from soundml_amd._tensor import OUT, STREAM, Batch, FramedStage, refuse_device_float64


class Entry:
    """a stand-in for a C entry: records every call's arguments, returns its status"""

    def __init__(self, status=0):
        self.calls, self.status = [], status

    def __call__(self, *args):
        self.calls.append(args)
        return self.status


def _faces():
    return (Entry(), Entry()), Entry()


def _run(x, shapes, host, device, **options):
    b = Batch(x, "op")
    return b, b.run(host, (7, b.ptr(), 3, OUT, OUT) if isinstance(shapes, list) else (7, b.ptr(), 3, OUT), device, (b.ptr(), OUT, STREAM), shapes, **options)


@pytest.mark.parametrize("dtype, which", [(np.float32, 0), (np.float64, 1)])
def test_host_entry_follows_the_width(dtype, which):
    host, device = _faces()
    x = np.arange(6, dtype=dtype).reshape(2, 3)
    b, out = _run(x, (2, 5), host, device)
    assert type(out) is np.ndarray and out.dtype == dtype and out.shape == (2, 5)
    assert len(host[which].calls) == 1 and not host[1 - which].calls and not device.calls
    seven, xp, three, op = host[which].calls[0]
    assert (seven, three) == (7, 3) and xp.value == b.data.ctypes.data and op.value == out.ctypes.data


def test_containers_and_integers():
    host, device = _faces()
    _, out = _run(torch.zeros(2, 3, dtype=torch.float64), (2, 4), host, device)
    assert isinstance(out, torch.Tensor) and not out.is_cuda and out.dtype == torch.float64 and tuple(out.shape) == (2, 4)
    assert len(host[1].calls) == 1
    b, out = _run(np.arange(6).reshape(2, 3), (2, 4), host, device)
    assert b.data.dtype == np.float32 and out.dtype == np.float32 and len(host[0].calls) == 1


def test_outputs_in_declared_order_and_null_for_none():
    host, device = _faces()
    x = np.zeros((2, 3), np.float32)
    _, (first, second) = _run(x, [(2, 1), (2, 9)], host, device)
    assert first.shape == (2, 1) and second.shape == (2, 9)
    assert [p.value for p in host[0].calls[0][3:]] == [first.ctypes.data, second.ctypes.data]
    _, (first, second) = _run(x, [None, (2, 9)], host, device)
    assert first is None and host[0].calls[1][3] is None and host[0].calls[1][4].value == second.ctypes.data
    _, out = _run(x, (0, 4), host, device, null_empty=True)
    assert out.shape == (0, 4) and host[0].calls[2][3] is None


@pytest.mark.parametrize("empty", ["zeros", "uninitialised"])
def test_an_empty_request_makes_no_call(empty):
    host, device = _faces()
    for x in (np.zeros((0, 3), np.float64), torch.zeros(0, 3, dtype=torch.float64)):
        _, (first, second) = _run(x, [(0, 1, 2), None], host, device, skip=True, empty=empty)
        assert type(first) is type(x) and tuple(first.shape) == (0, 1, 2) and second is None
        assert str(first.dtype).endswith("float64")
    _, out = _run(np.ones((2, 3), np.float32), (2, 1, 0), host, device, skip=True, empty=empty)
    assert out.shape == (2, 1, 0) and out.dtype == np.float32
    _, out = _run(np.ones((2, 3), np.float32), (2, 2), host, device, skip=True, empty=empty)
    assert np.array_equal(out, np.zeros((2, 2), np.float32))       # host outputs are zeros under either rule
    assert not host[0].calls and not host[1].calls and not device.calls


def test_a_status_raises_through_check():
    assert _lib.check(0) is None
    with pytest.raises(_lib.Failure):
        _run(np.zeros(3, np.float32), (3,), (Entry(_lib.SMX_FAILURE), Entry()), Entry())
    with pytest.raises(_lib.InvalidArgument):
        _run(np.zeros(3, np.float64), (3,), (Entry(), Entry(_lib.SMX_INVALID_ARGUMENT)), Entry())


def test_the_float64_refusal_words_what():
    class Resident:
        device, bytes = True, 8

    with pytest.raises(_lib.Failure, match=r"^op: device-resident float64 envelopes are not supported; pass a host array$"):
        refuse_device_float64("op", Resident(), "envelopes are")
    with pytest.raises(_lib.Failure, match=r"^op: device-resident float64 audio is not supported; pass a host array$"):
        refuse_device_float64("op", Resident())
    Resident.bytes = 4
    refuse_device_float64("op", Resident())
    Resident.device, Resident.bytes = False, 8
    refuse_device_float64("op", Resident())


# ---- FramedStage: the carry against the padded stream written out whole -------------------------------------------------------

class Recorder(FramedStage):
    def __init__(self, hop, border):
        super().__init__("recorder_stage", 8, hop, border)
        self.seen = []

    def _segment(self, samples, count):
        self.seen.append(np.array(samples.numpy() if isinstance(samples, torch.Tensor) else samples))
        return int(samples.shape[-1]), count


SIZES = [0, 2, 2, 1, 7, 20, 0, 1]        # border + 4 = one frame exactly (hop 11 then skips 3), chunks shorter than a frame, a long one


def _expected(sizes, frame_length, hop):
    """(length, count) | None per step and for flush: the frames complete in the padded stream so far, less those emitted"""
    border, padded, done, started, out = frame_length // 2, 0, 0, False, []
    for m in sizes + ["flush"]:
        if m == 0:
            out.append(None)
            continue
        if m == "flush":
            padded += border if started else 0
        else:
            padded, started = padded + m + (0 if started else border), True
        frames = 0 if padded < frame_length else 1 + (padded - frame_length) // hop
        out.append((padded - done * hop, frames - done) if frames > done else None)
        done = frames
    return out


@pytest.mark.parametrize("container", [np.asarray, torch.from_numpy], ids=["numpy", "torch"])
@pytest.mark.parametrize("border", ["zeros", "edge"])
@pytest.mark.parametrize("hop", [3, 11])
def test_framed_stage_frames_the_padded_stream(hop, border, container):
    x = np.arange(1, 2 * sum(SIZES) + 1, dtype=np.float32).reshape(2, -1)
    pad = np.zeros((2, 4), np.float32) if border == "zeros" else None
    whole = np.concatenate([x[:, :1].repeat(4, 1) if pad is None else pad, x, x[:, -1:].repeat(4, 1) if pad is None else pad], axis=1)
    stage = Recorder(hop, border)
    assert (stage.frame_length, stage.hop, stage.border, stage.latency, stage.rate, stage.name) == (8, hop, 4, 4, (1, hop), "recorder_stage")
    got, at = [], 0
    for m in SIZES:
        got.append(stage(container(x[:, at:at + m])))
        at += m
    flushed = stage.flush()
    assert got + [flushed[0] if flushed else None] == _expected(SIZES, 8, hop)
    first = 0                                 # every segment starts where its first frame does, and ends where the stream does
    for seg, (length, count) in zip(stage.seen, [e for e in _expected(SIZES, 8, hop) if e]):
        end = first * hop + length
        assert np.array_equal(seg, whole[:, first * hop:end])
        first += count
    assert hop != 11 or _expected(SIZES, 8, hop)[2:5] == [(8, 1), None, None]      # the skip outran a whole chunk
    assert stage.flush() == []
    with pytest.raises(_lib.InvalidArgument, match=r"^step: cannot feed a drained kernel \(flush consumed the tail; reset before reusing\)$"):
        stage.step(container(x[:, :1]))
    stage.reset()
    assert not stage._started and not stage._drained and stage._pending is None and stage._tail is None and stage._skip == 0
    assert stage.step(container(x[:, :3])) is None and stage._pending.shape == (2, 7)
