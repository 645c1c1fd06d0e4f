"""tengine_amd/csrc/block_pack.h, the weight blob of the fused bottleneck kernel (block_i8.hip), on the host: unpacking each of the
three panels by the documented A-fragment layout reproduces the OIHW weights, padding is zero (tests/csrc/block_pack_check.cc)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_unpacking_the_packed_panels_reproduces_oihw(tmp_path):
    exe = str(tmp_path / "block_pack_check")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fsanitize=address,undefined", "-I", os.path.join(ROOT, "tengine_amd", "csrc"),
                           os.path.join(ROOT, "tests", "csrc", "block_pack_check.cc"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "mismatches 0" in out.stdout, out.stdout + out.stderr
