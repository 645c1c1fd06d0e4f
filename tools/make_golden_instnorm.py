"""Writes tests/golden/instnorm_cases.npz: for every GPU case of tests/instnorm_helpers.py its seeded input and the outputs of the real
reference library, so that the tests have something to equal on a machine where oracle/_ref was never built.
tests/test_instnorm_cpu.py::test_golden_is_the_real_reference checks the file against the reference wherever that exists.

    python tools/make_golden_instnorm.py          (needs oracle/_ref/libtengine-lite.so)
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import instnorm_helpers as nh  # noqa: E402
from oracle import ref_capi as ref  # noqa: E402


def main():
    assert ref.available(), "build the reference library first (oracle/build_ref.py)"
    z = {}
    for case, build in sorted(nh.gpu_cases().items()):
        g, x = build()
        z.update(nh.golden_entry(case, x, nh.reference_outputs(ref, g, x)))
    np.savez_compressed(nh.GOLDEN, **z)
    print(nh.GOLDEN, os.path.getsize(nh.GOLDEN), "bytes,", len(z), "arrays")


if __name__ == "__main__":
    main()
