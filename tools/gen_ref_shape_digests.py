#!/usr/bin/env python3
"""Generates tests/golden/resample/ref_shape_digests.json: what the reference's own compiled `soundml_resample_shape_run`
(oracle/_ref/libresample_shape_ref.so, built by `make -C oracle` where the reference's source is present) returns on the
inputs of tests/test_fir_oracle_pins.py::test_ols_shape_identity and
tests/test_gpu_parity.py::test_resample_shape_is_the_reference_stub_bit_for_bit.

The tests rebuild the same inputs (seeded numpy), check them against the stored input digest, and hold their results against
the stored output digest: bit for bit the reference's values, without the reference.  Digests are SHA-256 of the complex128
bytes with every -0.0 made +0.0 (conftest.shape_digest), so that equal digests mean exactly what np.array_equal meant.
Run from the repo root.
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import shape_digest               # noqa: E402
from oracle import c_oracle, soundml_oracle as O  # noqa: E402

CASES = [(1, 1), (2, 1), (3, 1), (4, 1), (1, 2), (1, 3), (1, 4)]


def cpu_inputs(l, m):
    """test_ols_shape_identity's inputs"""
    rng = np.random.default_rng(100 * l + m)
    n = 96 if m == 3 else 64
    k = 5
    proto = rng.uniform(-1, 1, size=2 * k * l + 1)
    x = rng.uniform(-1, 1, size=(3, n))
    return np.fft.rfft(x, axis=-1), O.ols_plan_spectrum(proto, n, l, m), n


def gpu_inputs(l, m):
    """test_resample_shape_is_the_reference_stub_bit_for_bit's inputs"""
    rng = np.random.default_rng(7 * l + m)
    n = 96 if m == 3 else 2048
    k = 5
    proto = rng.uniform(-1, 1, size=2 * k * l + 1)
    oh = O.ols_plan_spectrum(proto, n, l, m)
    return np.fft.rfft(rng.uniform(-1, 1, size=(9, n)), axis=-1), oh, n


def main():
    c_oracle.build()
    if not c_oracle.have_ref():
        raise SystemExit("oracle/_ref/libresample_shape_ref.so is missing: build it with `make -C oracle` where the reference is present")
    out = {"generator": "tools/gen_ref_shape_digests.py", "numpy": np.__version__,
           "digest": "sha256 of the complex128 bytes, -0.0 made +0.0 (tests/conftest.py shape_digest)"}
    for suite, make in (("cpu", cpu_inputs), ("gpu", gpu_inputs)):
        rows = {}
        for l, m in CASES:
            spec, oh, n = make(l, m)
            ref = c_oracle.ref_resample_shape(spec, oh, n, l, m)
            # the C restatement the tests also compute must agree under the digest as it does under np.array_equal
            assert shape_digest(ref) == shape_digest(c_oracle.resample_shape(spec, oh, n, l, m)), (suite, l, m)
            rows["%d-%d" % (l, m)] = {"input": shape_digest(spec, oh), "output": shape_digest(ref), "shape": list(ref.shape)}
        out[suite] = rows
    path = os.path.join(ROOT, "tests", "golden", "resample", "ref_shape_digests.json")
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print("wrote", path)


if __name__ == "__main__":
    main()
