"""The census of libhypergen_frag.so (tests/frag_census.py) against the built library, on the CPU: every kernel `nm -C` lists has
exactly one row and every row names a kernel that exists; hg_frag_kernel_names() lists the same names in the same order; and
the four other libraries, whose own censuses are closed, hold none of them."""
import pytest

import frag_census as fc
import library_kernels as lk


@pytest.fixture(scope="module")
def hg():
    import hypergen_amd
    hypergen_amd.lib_frag()
    return hypergen_amd


def test_census_equals_the_library(hg):
    lib = lk.all_kernels(hg.FRAG_LIB_PATH)
    names = [r.name for r in fc.ROWS]
    print("%d kernels in libhypergen_frag.so, %d census rows" % (len(lib), len(names)))
    assert len(set(names)) == len(names) and len(set(lib)) == len(lib)
    assert sorted(names) == lib


def test_rows_are_what_the_library_reports_in_launch_order(hg):
    assert [r.name for r in fc.ROWS] == hg.frag_kernel_names()
    assert list(hg.frag_launch_counts()) == hg.frag_kernel_names()
    for r in fc.ROWS:
        assert r.entries and all(e in hg.FRAG_EXPORTS for e in r.entries)
        assert lk.family(r.name) == r.name and r.name.startswith("frag_")


def test_the_other_libraries_hold_no_fragment_kernel(hg):
    hg.lib_aa(), hg.lib_tx(), hg.lib_rec()
    for path in (hg.LIB_PATH, hg.AA_LIB_PATH, hg.TX_LIB_PATH, hg.REC_LIB_PATH):
        assert not [n for n in lk.all_kernels(path) if lk.family(n).startswith("frag_")]
    assert not [n for n in lk.all_kernels(hg.FRAG_LIB_PATH) if not lk.family(n).startswith("frag_")]
