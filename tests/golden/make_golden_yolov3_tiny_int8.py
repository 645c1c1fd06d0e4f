"""Generates tests/golden/yolov3_tiny_int8_416_seed3.npz: the two head outputs of the REAL reference (oracle/_ref, built from the
unmodified reference sources by oracle/build_ref.py) for the seeded int8 YOLOv3-tiny at 416 x 416, batch 1 -- the int8 twin of
yolov3_tiny_uint8_416_seed3.npz (make_golden.py).  Run where the reference sources exist:
    python tests/golden/make_golden_yolov3_tiny_int8.py
The model is re-synthesised from its seed and the committed calibration table (tengine_amd/calib/yolov3_tiny_int8.json)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import build_ref, ref_capi  # noqa: E402
from tengine_amd import models, tm2     # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "yolov3_tiny_int8_416_seed3.npz")


def reference_outputs(threads=None):
    g = models.build("yolov3_tiny", "int8", 1)
    x = models.synth_input(g, 3)
    return ref_capi.run_model(tm2.write_tm2(g), x, ref_capi.MODE_INT8, threads or min(16, os.cpu_count() or 1))


def main():
    build_ref.build()
    outs = reference_outputs()
    np.savez_compressed(PATH, **{"out%d" % i: o for i, o in enumerate(outs)})
    print(PATH, [o.shape for o in outs], [str(o.dtype) for o in outs], [len(np.unique(o)) for o in outs])


if __name__ == "__main__":
    main()
