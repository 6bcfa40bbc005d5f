"""The census of support kernels (tests/select_census.py) against the built library, on the CPU: every hit-list, radix-sort,
search-selection, dist-prepass, listed-pair, logf, ANI-from-dots and publishing kernel instantiation the library holds has
exactly one row, and every row names an instantiation that exists.  (test_gpu_select_census.py runs the rows.)"""
import re

import pytest

import library_kernels as lk
import select_census as sc

# families, not names: a gather_keys_kernel<5>, a radix_merge_kernel, a search_topk_fold_kernel or a prep_fp8_kernel needs a
# row too
FAMILIES = re.compile(r"(?:gather_keys|permute_hits|topk|fill_empty|radix_[a-z0-9_]+|search_[a-z0-9_]+|prep(?:_[a-z0-9]+)*"
                      r"|decide(?:_[a-z0-9]+)*|unpack_meta|ani_pairs[a-z0-9_]*|logf|ani_from_dots|publish_[a-z0-9_]+)_kernel(?:<[^>]*>)?")
# nm leaves these three mangled (a _Float16 * parameter): a listing that drops them must not pass
MANGLED = ("prep_kernel", "prep_fast_kernel", "prep_cen_kernel")


@pytest.fixture(scope="module")
def hg():
    import hypergen_amd
    hypergen_amd.lib()
    return hypergen_amd


def library_kernels(hg):
    return [n for n in lk.all_kernels(hg.LIB_PATH) if FAMILIES.fullmatch(n)]


def test_census_equals_the_library(hg):
    lib = library_kernels(hg)
    assert len(set(lib)) == len(lib), "two stubs of one spelling"
    lib = set(lib)
    for name in MANGLED:
        assert name in lib, "the listing lost %s" % name
    names = [r.name for r in sc.ROWS]
    dup = sorted({n for n in names if names.count(n) > 1})
    assert not dup, "rows listed twice: %s" % dup
    for r in sc.ROWS:
        if r.unreachable is not None:
            print("unreachable: %s -- %s" % (r.name, r.unreachable))
    missing = sorted(lib - set(names))
    stale = sorted(set(names) - lib)
    assert not missing, "instantiations in the library without a census row: %s" % missing
    assert not stale, "census rows whose kernel the library does not contain: %s" % stale
    assert len(lib) == len(names) == 29


def test_census_families_are_complete():
    """the table's own shape: 15 hit-list kernels (5 key gathers, 3 + 1 + 3 of the radix sort, 4 others), 3 of the search, 7
    of the dist prepasses, 4 others"""
    h = [r.name for r in sc.HITS_ROWS]
    assert [n for n in h if n.startswith("gather_keys")] == ["gather_keys_kernel<%d>" % w for w in range(5)]
    kd = ["<unsigned int, false>", "<unsigned int, true>", "<unsigned long, true>"]
    assert [n for n in h if n.startswith("radix_hist")] == ["radix_hist_kernel" + a for a in kd]
    assert [n for n in h if n.startswith("radix_scatter")] == ["radix_scatter_kernel" + a for a in kd]
    assert sorted(n for n in h if "<" not in n) == ["fill_empty_kernel", "permute_hits_kernel", "radix_scan_kernel", "topk_kernel"]
    assert len(h) == 15
    assert sorted(r.name for r in sc.SEARCH_ROWS) == ["search_topk_%s_kernel" % s for s in ("emit", "merge", "select")]
    assert sorted(r.name for r in sc.PREP_ROWS) == ["decide_cen_kernel", "decide_kernel", "prep_cen_kernel", "prep_fast_kernel",
                                                    "prep_i8_kernel", "prep_kernel", "unpack_meta_kernel"]
    assert sorted(r.name for r in sc.OTHER_ROWS) == ["ani_from_dots_kernel", "ani_pairs_kernel", "logf_kernel", "publish_words_kernel"]
    assert len(sc.ROWS) == 29
    assert {r.entry for r in sc.ROWS} == set(sc.ENTRIES)
    for r in sc.ROWS:
        assert r.entry in sc.ENTRIES and r.inputs and len(r) == 5, r
        assert set(r.debug) <= {"dist_path"}, r
        assert (r.entry == "dist") == ("dist_path" in r.debug), r  # a prepass row names the operand form it prepares
        assert FAMILIES.fullmatch(r.name), r


def test_stub_names_are_read_from_both_forms():
    """the listing's own parser: demangled with and without template arguments, at file scope, and the mangled form nm leaves"""
    assert lk.stub_name("(anonymous namespace)::__device_stub__topk_kernel(hg_ani_hit const*, unsigned int)") == "topk_kernel"
    assert lk.stub_name("void (anonymous namespace)::__device_stub__radix_hist_kernel<unsigned long, true>(unsigned long const*)") == \
        "radix_hist_kernel<unsigned long, true>"
    assert lk.stub_name("__device_stub__expand_bits_kernel(unsigned int const*, unsigned int)") == "expand_bits_kernel"
    assert lk.stub_name("_ZN12_GLOBAL__N_126__device_stub__prep_kernelEPKsjjjjPDF16_Py") == "prep_kernel"
    assert lk.stub_name("_ZN12_GLOBAL__N_131__device_stub__prep_fast_kernelEPKsjjjjPDF16_PyjPKj") == "prep_fast_kernel"
    assert lk.stub_name("_Z26__device_stub__prep_kernelPKsPDF16_") == "prep_kernel"  # (file scope: no nested name)
    with pytest.raises(ValueError):
        lk.stub_name("_ZN12_GLOBAL__N_126__device_stub__prep_kernelILi3EEvPKsPDF16_")
    with pytest.raises(ValueError):
        lk.stub_name("_ZN3foo__device_stub__")
