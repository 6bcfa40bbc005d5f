"""The host-side C++ of neighbour joining under AddressSanitizer + UBSan on the CPU build, as a stand-alone program:
hg_nj_math.h -- the three formulas the kernels of hg_nj.hip use -- at 65 536 live nodes with every distance at its maximum
and at 0, the floor of negative numerators and Q within 2^50, against 128-bit arithmetic; and hg_nj_newick (hg_formats.cpp)
on random valid join lists, lists broken in one place and random garbage."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_nj_math_and_newick_under_asan_ubsan(tmp_path):
    exe = tmp_path / "nj_driver"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", os.path.join(ROOT, "tests", "native", "nj_driver.cpp"),
                           os.path.join(ROOT, "hyper-gen_amd", "csrc", "hg_formats.cpp"), "-I", os.path.join(ROOT, "include"),
                           "-lz", "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "nj driver ok" in out.stdout, out.stdout + out.stderr
