"""The field packer that tri_format_kernel runs per element (hg_tri_field, hg_tri.h) under AddressSanitizer + UBSan on the CPU, as
a stand-alone program: every m in 0..100 000 against snprintf("%7.3f") of m / 1000, under both separators."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_field_is_what_printf_writes(tmp_path):
    exe = tmp_path / "tri_format_driver"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", os.path.join(ROOT, "tests", "native", "tri_format_driver.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    last = out.stdout.splitlines()[-1].split()
    assert last[:4] == ["tri", "format", "driver", "ok:"] and last[-2:] == ["0", "wrong"], out.stdout
    assert int(last[4]) == 2 * 100_001
