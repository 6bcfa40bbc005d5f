"""The census of libhypergen_tx.so (tests/tx_census.py) against the built library, on the CPU: every kernel instantiation
`nm -C` lists has exactly one row and every row names an instantiation that exists -- and neither other library, whose own
censuses are closed (test_census_cover.py, test_aa_census.py), holds one of them."""
import pytest

import library_kernels as lk
import tx_census as tc


@pytest.fixture(scope="module")
def hg():
    import hypergen_amd
    hypergen_amd.lib_tx()
    return hypergen_amd


def test_census_equals_the_library(hg):
    lib = lk.all_kernels(hg.TX_LIB_PATH)
    names = [r.name for r in tc.ROWS]
    print("%d kernel instantiations in libhypergen_tx.so, %d census rows" % (len(lib), len(names)))
    assert len(set(names)) == len(names) and len(set(lib)) == len(lib)
    assert sorted(names) == lib


def test_rows_partition_the_ksizes_and_name_what_the_library_reports(hg):
    assert len(tc.ROWS) == 4
    seen = [k for r in tc.ROWS for k in r.ksizes]
    assert sorted(seen) == list(range(1, 33)) and len(set(seen)) == 32
    for r in tc.ROWS:
        assert lk.family(r.name) == "tx_kmer_sample_kernel" and r.entries == tc.ENTRIES
        for k in r.ksizes:
            assert hg.tx_kernel_name(k) == r.name
        for e in r.entries:
            assert e in hg.TX_EXPORTS


def test_the_other_libraries_hold_no_translated_kernel(hg):
    for path in (hg.LIB_PATH, hg.AA_LIB_PATH):
        assert not [n for n in lk.all_kernels(path) if lk.family(n).startswith("tx_")]
    assert not [n for n in lk.all_kernels(hg.TX_LIB_PATH) if not lk.family(n).startswith("tx_")]
