"""The census of libhypergen_aa.so (tests/aa_census.py) against the built library, on the CPU: every kernel instantiation
`nm -C` lists has exactly one row and every row names an instantiation that exists -- and the nucleotide library, whose own
census is closed (test_census_cover.py), holds none of them."""
import pytest

import aa_census as ac
import library_kernels as lk


@pytest.fixture(scope="module")
def hg():
    import hypergen_amd
    hypergen_amd.lib_aa()
    return hypergen_amd


def test_census_equals_the_library(hg):
    lib = lk.all_kernels(hg.AA_LIB_PATH)
    names = [r.name for r in ac.ROWS]
    print("%d kernel instantiations in libhypergen_aa.so, %d census rows" % (len(lib), len(names)))
    assert len(set(names)) == len(names) and len(set(lib)) == len(lib)
    assert sorted(names) == lib


def test_rows_partition_the_ksizes_and_name_what_the_library_reports(hg):
    assert len(ac.ROWS) == 4
    seen = [k for r in ac.ROWS for k in r.ksizes]
    assert sorted(seen) == list(range(1, 33)) and len(set(seen)) == 32
    for r in ac.ROWS:
        assert lk.family(r.name) == "aa_kmer_sample_kernel" and r.entries == ac.ENTRIES
        for k in r.ksizes:
            assert hg.aa_kernel_name(k) == r.name
        for e in r.entries:
            assert e in hg.AA_EXPORTS


def test_the_main_library_holds_no_amino_acid_kernel(hg):
    assert not [n for n in lk.all_kernels(hg.LIB_PATH) if lk.family(n).startswith("aa_")]
