"""The division by the bin width that hist_count_kernel performs per element (hg_hist_magic / hg_hist_div, hg_hist.h) under
AddressSanitizer + UBSan on the CPU, as a stand-alone program: every bin edge b w and b w - 1 of every width w in 1..100 000
against the plain integer division -- the helper is monotone in m, so the edges suffice."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bin_division_is_exact_at_every_edge_of_every_width(tmp_path):
    exe = tmp_path / "hist_div_driver"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", os.path.join(ROOT, "tests", "native", "hist_div_driver.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    last = out.stdout.splitlines()[-1].split()
    assert last[:4] == ["hist", "div", "driver", "ok:"] and last[-2:] == ["0", "wrong"], out.stdout
    # the edges of all widths: sum over w of 2 (100 000 // w) + 2
    assert int(last[4]) == sum(2 * (100_000 // w) + 2 for w in range(1, 100_001)) and int(last[4]) > 2_400_000
