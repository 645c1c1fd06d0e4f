"""Writes tests/golden/slice_cases.npz: for every GPU case of tests/slice_op_helpers.py (seeded inputs) the outputs of the real reference
library -- bytes and shapes; shape and SHA-256 for the one large case -- and, under "table__<id>", the 256 bytes the reference's uint8
Slice makes of the byte values 0 .. 255 for every parameter pair of TABLE_SETS, so that the tests have something to equal on a machine
where oracle/_ref was never built.  tests/test_slice_cpu.py::test_golden_is_the_real_reference checks the file against the reference
wherever that exists.

    python tools/make_golden_slice.py          (needs oracle/_ref/libtengine-lite.so)
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import slice_op_helpers as so  # noqa: E402
from oracle import ref_capi as ref  # noqa: E402


def main():
    assert ref.available(), "build the reference library first (oracle/build_ref.py)"
    z = {}
    for case, build in sorted(so.gpu_cases().items()):
        g, x = build()
        z.update(so.golden_entry(case, so.reference_outputs(ref, g, x)))
    for name, in_q, out_q in so.TABLE_SETS:
        g, x = so.table_case(in_q, out_q)
        z["table__" + name] = so.reference_outputs(ref, g, x)[0].reshape(-1)
    np.savez_compressed(so.GOLDEN, **z)
    print(so.GOLDEN, os.path.getsize(so.GOLDEN), "bytes,", len(z), "arrays")


if __name__ == "__main__":
    main()
