"""The census of libhypergen_hist.so (tests/hist_census.py) against the built library, on the CPU: every kernel `nm -C` lists has
exactly one row and every row names a kernel that exists; hg_hist_kernel_names() lists the same names in the same order; and
the five other libraries, whose own censuses are closed, hold none of them."""
import pytest

import hist_census as hc
import library_kernels as lk


@pytest.fixture(scope="module")
def hg():
    import hypergen_amd
    hypergen_amd.lib_hist()
    return hypergen_amd


def test_census_equals_the_library(hg):
    lib = lk.all_kernels(hg.HIST_LIB_PATH)
    names = [r.name for r in hc.ROWS]
    print("%d kernels in libhypergen_hist.so, %d census rows" % (len(lib), len(names)))
    assert len(set(names)) == len(names) and len(set(lib)) == len(lib)
    assert sorted(names) == lib


def test_rows_are_what_the_library_reports(hg):
    assert [r.name for r in hc.ROWS] == hg.hist_kernel_names()
    assert list(hg.hist_launch_counts()) == hg.hist_kernel_names()
    for r in hc.ROWS:
        assert r.entries and all(e in hg.HIST_EXPORTS for e in r.entries)
        assert lk.family(r.name) == r.name and r.name.startswith("hist_")


def test_the_other_libraries_hold_no_histogram_kernel(hg):
    hg.lib_aa(), hg.lib_tx(), hg.lib_rec(), hg.lib_frag()
    for path in (hg.LIB_PATH, hg.AA_LIB_PATH, hg.TX_LIB_PATH, hg.REC_LIB_PATH, hg.FRAG_LIB_PATH):
        assert not [n for n in lk.all_kernels(path) if lk.family(n).startswith("hist_")]
    assert not [n for n in lk.all_kernels(hg.HIST_LIB_PATH) if not lk.family(n).startswith("hist_")]
