"""Writes tests/golden/d2s_cases.npz: for every GPU case of tests/d2s_helpers.py its seeded input and the outputs of the real reference
library, so that the tests have something to equal on a machine where oracle/_ref was never built.
tests/test_d2s_cpu.py::test_golden_is_the_real_reference checks the file against the reference wherever that exists.

    python tools/make_golden_d2s.py          (needs oracle/_ref/libtengine-lite.so)
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import d2s_helpers as dh  # noqa: E402
from oracle import ref_capi as ref  # noqa: E402


def main():
    assert ref.available(), "build the reference library first (oracle/build_ref.py)"
    z = {}
    for case, (dtype, build) in sorted(dh.gpu_cases().items()):
        g, x = build()
        z.update(dh.golden_entry(case, x, dh.reference_outputs(ref, g, x, dtype)))
    np.savez_compressed(dh.GOLDEN, **z)
    print(dh.GOLDEN, os.path.getsize(dh.GOLDEN), "bytes,", len(z), "arrays")


if __name__ == "__main__":
    main()
