"""The arithmetic behind a graph's two slots (tengine_amd/csrc/graph_slots.h), on the host: which written ranges merge into which
private spans, and which 8-byte argument words of a recorded launch move into slot 1's copy (tests/csrc/slot_rebase_check.cc)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_slot_spans_and_argument_rebase(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
        cxx = hipcc if (os.path.exists(hipcc) or shutil.which(hipcc)) else None
    if cxx is None:
        pytest.skip("no C++ compiler available")
    exe = str(tmp_path / "slot_rebase_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "tengine_amd", "csrc"),
                           os.path.join(ROOT, "tests", "csrc", "slot_rebase_check.cc"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "0 failures" in out.stdout, out.stdout
