"""Resample.Config on the host (no device): the plan of resample.ml:872-939 against the oracle's restatement of the
single-stage design, the accessors of resample.ml:1021-1056, Config.equal, and the reference's Invalid_argument wording."""
import math

import numpy as np
import pytest

from oracle import resample_metrics as M
from oracle import soundml_oracle as O

import soundml_amd as S
from soundml_amd import Resample


def test_the_documented_plans():
    """resample.mli:146-147: 44100 -> 48000 is 160/147 at K = 95, 44100 -> 16000 is 160/441 at K = 261 (`High)."""
    for sr, target, want in ((44100, 48000, (160, 147, 95)), (44100, 16000, (160, 441, 261))):
        c = Resample.Config.create(sr, target)
        assert c.rate + (c.latency,) == want
        assert (c.sample_rate, c.target, c.quality) == (sr, target, "high")
        assert c.executor == "direct"


@pytest.mark.parametrize("sr,target,quality", [(44100, 48000, "fast"), (44100, 48000, "best"), (44100, 16000, "fast"),
                                               (44100, 16000, "best"), (48000, 44100, "high"), (48000, 44100, "fast"),
                                               (11025, 192000, "high"), (11025, 192000, "best"), (192000, 11025, "high")])
def test_plan_and_prototype_equal_the_oracle(sr, target, quality):
    g = math.gcd(sr, target)
    l, m = target // g, sr // g
    k, fc, beta = M.single_stage(l, m, quality)
    c = Resample.Config.create(sr, target, quality)
    assert (c.rate, c.latency) == ((l, m), k)
    assert c.design == (fc, beta)
    proto = c.prototype()
    assert proto.dtype == np.float64 and proto.shape == (2 * k * l + 1,)
    assert np.array_equal(proto, O.resample_prototype(l, k, fc, beta))
    proto[:] = 0.0                                              # a fresh copy each time
    assert np.array_equal(c.prototype(), O.resample_prototype(l, k, fc, beta))


def test_l_2560():
    assert Resample.Config.create(11025, 192000).rate == (2560, 147)


def test_a_custom_spec_plans_as_its_numbers():
    c = Resample.Config.create(44100, 48000, Resample.Spec(126.0, 0.913))
    h = Resample.Config.create(44100, 48000, "high")
    assert (c.rate, c.latency) == (h.rate, h.latency) and np.array_equal(c.prototype(), h.prototype())
    assert c.quality == S.Spec(126.0, 0.913)


@pytest.mark.parametrize("sr,target", [(44100, 48000), (48000, 44100), (44100, 16000), (3, 2), (7, 7)])
def test_output_frames_and_latency(sr, target):
    c = Resample.Config.create(sr, target)
    l, m = c.rate
    for n in (0, 1, m - 1, m, m + 1, 44100):
        assert c.output_frames(n) == -(-n * l // m)
    with pytest.raises(S.InvalidArgument, match="cannot resample a signal of length -1"):
        c.output_frames(-1)
    num, den = c.output_latency
    assert math.gcd(num, den) == 1 and num * m == c.latency * l * den
    if c.latency == 0:
        assert (num, den) == (0, 1)


def test_identity():
    c = Resample.Config.create(48000, 48000)
    assert (c.rate, c.latency, c.executor, c.output_latency) == ((1, 1), 0, "identity", (0, 1))
    assert np.array_equal(c.prototype(), [1.0])
    assert c.output_frames(17) == 17


def test_executors():
    """resample.ml:951: overlap-save exactly for the pure x2..4 and /2..4 conversions."""
    assert Resample.Config.create(48000, 16000).executor == "ols"
    assert Resample.Config.create(16000, 48000).executor == "ols"
    assert Resample.Config.create(24000, 48000).executor == "ols"
    assert Resample.Config.create(48000, 12000).executor == "ols"
    assert Resample.Config.create(44100, 48000).executor == "direct"
    assert Resample.Config.create(48000, 8000).executor == "direct"      # /6: past the overlap-save classes
    assert Resample.Config.create(8000, 40000).executor == "direct"      # x5
    assert Resample.Config.create(3, 2).executor == "direct"


def test_equal():
    """Config.equal (resample.ml:1139-1150): rates and quality; a custom spec never equals a named quality."""
    a = Resample.Config.create(44100, 48000)
    assert a == Resample.Config.create(44100, 48000, "high")
    assert a != Resample.Config.create(44100, 48000, "fast")
    assert a != Resample.Config.create(48000, 44100)
    assert a != Resample.Config.create(44100, 16000)
    assert a != Resample.Config.create(44100, 48000, Resample.Spec(126.0, 0.913))
    assert Resample.Config.create(44100, 48000, Resample.Spec(90.0, 0.9)) == Resample.Config.create(44100, 48000, Resample.Spec(90.0, 0.9))
    assert Resample.Config.create(44100, 48000, Resample.Spec(90.0, 0.9)) != Resample.Config.create(44100, 48000, Resample.Spec(90.0, 0.91))
    assert Resample.Config.create(88200, 96000) != a                     # the same L / M, other rates


def test_repr_names_the_plan():
    r = repr(Resample.Config.create(44100, 48000))
    assert "\n" not in r
    for part in ("44100", "48000", "160/147", "K=95", "direct"):
        assert part in r


@pytest.mark.parametrize("args,phrase", [
    ((0, 48000), "cannot resample from 0 Hz (sample_rate must be at least 1)"),
    ((44100, 0), "cannot resample to 0 Hz (target must be at least 1)"),
    ((0, 0), "cannot resample from 0 Hz"),                               # the order of resample.ml:873-881
    ((44100, 48000, Resample.Spec(39.9, 0.9)), "39.9 dB of stop-band rejection (attenuation must be finite, in [40, 200])"),
    ((44100, 48000, Resample.Spec(float("inf"), 0.9)), "attenuation must be finite"),
    ((44100, 48000, Resample.Spec(100.0, 0.995)), "cannot preserve 0.995 of the band (passband must be finite, in [0.5, 0.99])"),
    ((44100, 0, Resample.Spec(39.9, 0.995)), "cannot resample to 0 Hz"),
    ((44100, 48000, Resample.Spec(39.9, 0.995)), "stop-band rejection"),
])
def test_validation_messages(args, phrase):
    with pytest.raises(S.InvalidArgument) as e:
        Resample.Config.create(*args)
    assert phrase in str(e.value) and str(e.value).startswith("create: ")


def test_over_budget_messages():
    """resample.ml:997-1011: the message names the rates, L, the bank and the budget; the clock-drift hint only near unity."""
    with pytest.raises(S.InvalidArgument) as e:
        Resample.Config.create(44100, 44099)
    text = str(e.value)
    for part in ("cannot resample 44100 Hz to 44099 Hz", "44099 phases need a", "MB bank", "the budget is 8 MB",
                 "hint: near-unity conversion is clock-drift correction"):
        assert part in text, text
    with pytest.raises(S.InvalidArgument) as e:
        Resample.Config.create(44100, 16000, Resample.Spec(200.0, 0.99))
    text = str(e.value)
    for part in ("cannot resample 44100 Hz to 16000 Hz", "160 phases need a 9.0 MB bank", "the budget is 8 MB"):
        assert part in text, text
    assert "hint" not in text and "clock-drift" not in text
