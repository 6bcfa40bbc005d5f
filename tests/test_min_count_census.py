"""The census of min_count_* kernels (tests/min_count_census.py) against the built library, on the CPU.  (test_gpu_min_count.py
runs the rows.)"""
import re
import subprocess

import pytest

import min_count_census as mc
import set_encode_census as sc

FAMILY = re.compile(r"::(min_count_[a-z_]*(?:<[^>()]*>)?)\(")


@pytest.fixture(scope="module")
def hg():
    import hypergen_amd
    hypergen_amd.lib()
    return hypergen_amd


def test_census_equals_the_library(hg):
    nm = subprocess.run(["nm", "-C", hg.LIB_PATH], capture_output=True, text=True, check=True).stdout
    lib = set(FAMILY.findall(nm))
    names = [r.name for r in mc.ROWS]
    assert len(set(names)) == len(names)
    assert not sorted(lib - set(names)), "instantiations in the library without a census row"
    assert not sorted(set(names) - lib), "census rows whose kernel the library does not contain"
    assert len(lib) == 5


def test_rows_are_routed_and_twinned(hg):
    first = {r.name: r for r in sc.ROWS}
    for r in mc.ROWS:
        assert r.entry in mc.ENTRIES and r.inputs and r.unreachable is None, r
        assert set(r.debug) <= {"sort_test_buckets", "sketch_path"}, r
        # the twin is a set-stage kernel of the first family, reached by the same entry under the same debug keys
        assert r.twin in first and first[r.twin].entry == r.entry and first[r.twin].debug == r.debug, r
    assert len({r.twin for r in mc.ROWS}) == len(mc.ROWS)


def test_launch_lists_swap_the_twins_only():
    chain = ["bucket_count_kernel", "bucket_scan_kernel", "bucket_scatter_kernel", "bucket_sort_kernel", "bucket_scan_kernel",
             "bucket_copy_kernel", "sort_unique_kernel<false>"]
    assert mc.sort_launches(chain, 1) == chain and mc.sort_launches(chain, 0) == chain
    assert mc.sort_launches(chain, 2) == ["bucket_count_kernel", "bucket_scan_kernel", "bucket_scatter_kernel",
                                          "min_count_bucket_kernel", "bucket_scan_kernel", "bucket_copy_kernel",
                                          "min_count_kernel<false>"]
    assert mc.sort_launches(["sort_unique_wave_kernel", "sort_unique_rest_kernel"], 5) == ["min_count_wave_kernel",
                                                                                            "min_count_rest_kernel"]
