"""Writes tests/golden/resize_cases.npz: for every GPU case of tests/resize_helpers.py its seeded input and the outputs of the real
reference library, so that the tests have something to equal on a machine where oracle/_ref was never built.
tests/test_resize_cpu.py::test_golden_is_the_real_reference checks the file against the reference wherever that exists.

    python tools/make_golden_resize.py          (needs oracle/_ref/libtengine-lite.so)
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import resize_helpers as rh  # noqa: E402
from oracle import ref_capi as ref  # noqa: E402


def main():
    assert ref.available(), "build the reference library first (oracle/build_ref.py)"
    z = {}
    for case, (dtype, build) in sorted(rh.gpu_cases().items()):
        g, x = build()
        z.update(rh.golden_entry(case, x, rh.reference_outputs(ref, g, x, dtype)))
    np.savez_compressed(rh.GOLDEN, **z)
    print(rh.GOLDEN, os.path.getsize(rh.GOLDEN), "bytes,", len(z), "arrays")


if __name__ == "__main__":
    main()
