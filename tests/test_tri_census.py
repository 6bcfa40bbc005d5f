"""The census of libhypergen_tri.so (tests/tri_census.py) against the built library, on the CPU: every kernel `nm -C` lists has
exactly one row and every row names a kernel that exists; hg_tri_kernel_names() lists the same names in the same order; and
the six other libraries, whose own censuses are closed, hold none of them."""
import pytest

import library_kernels as lk
import tri_census as tc


@pytest.fixture(scope="module")
def hg():
    import hypergen_amd
    hypergen_amd.lib_tri()
    return hypergen_amd


def test_census_equals_the_library(hg):
    lib = lk.all_kernels(hg.TRI_LIB_PATH)
    names = [r.name for r in tc.ROWS]
    print("%d kernels in libhypergen_tri.so, %d census rows" % (len(lib), len(names)))
    assert len(set(names)) == len(names) and len(set(lib)) == len(lib)
    assert sorted(names) == lib


def test_rows_are_what_the_library_reports(hg):
    assert [r.name for r in tc.ROWS] == hg.tri_kernel_names()
    assert list(hg.tri_launch_counts()) == hg.tri_kernel_names()
    for r in tc.ROWS:
        assert r.entries and all(e in hg.TRI_EXPORTS for e in r.entries)
        assert lk.family(r.name) == r.name and r.name.startswith("tri_")


def test_the_other_libraries_hold_no_triangle_kernel(hg):
    hg.lib_aa(), hg.lib_tx(), hg.lib_rec(), hg.lib_frag(), hg.lib_hist()
    for path in (hg.LIB_PATH, hg.AA_LIB_PATH, hg.TX_LIB_PATH, hg.REC_LIB_PATH, hg.FRAG_LIB_PATH, hg.HIST_LIB_PATH):
        assert not [n for n in lk.all_kernels(path) if lk.family(n).startswith("tri_")]
    assert not [n for n in lk.all_kernels(hg.TRI_LIB_PATH) if not lk.family(n).startswith("tri_")]
