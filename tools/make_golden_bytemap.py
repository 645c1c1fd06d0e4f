"""Writes tests/golden/bytemap_cases.npz: for every GPU case of tests/bytemap_helpers.py (seeded inputs) the inputs and the outputs of
the real reference library, so that the GPU tests have something to equal on a machine where oracle/_ref was never built.
tests/test_bytemap_cpu.py::test_golden_is_the_real_reference checks the file against the reference wherever that exists.

    python tools/make_golden_bytemap.py          (needs oracle/_ref/libtengine-lite.so)
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import bytemap_helpers as bh  # noqa: E402
from oracle import ref_capi as ref  # noqa: E402


def main():
    assert ref.available(), "build the reference library first (oracle/build_ref.py)"
    z = {}
    for case, (dtype, build) in sorted(bh.gpu_cases().items()):
        g, xs = build()
        z.update(bh.golden_entry(case, xs, bh.reference_outputs(ref, g, xs, dtype)))
    np.savez_compressed(bh.GOLDEN, **z)
    print(bh.GOLDEN, os.path.getsize(bh.GOLDEN), "bytes,", len(z), "arrays")


if __name__ == "__main__":
    main()
