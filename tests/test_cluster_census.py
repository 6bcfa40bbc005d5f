"""The census of clustering, tree and statistics kernels (tests/cluster_census.py) against the built library, on the CPU: every
cluster_*, greedy_*, setcover_*, tree_*, average_*, complete_*, cluster_stats_* and nj_* kernel instantiation the library holds
has exactly one row, and every row names an instantiation that exists.  (test_gpu_cluster_census.py runs the rows.)"""
import re

import pytest

import cluster_census as cc
import library_kernels as lk

# families, not names: a greedy_prune_kernel or an nj_fold_kernel<4> needs a row too
FAMILIES = re.compile(r"(cluster_stats|cluster|greedy|setcover|tree|average|complete|nj)_[a-z0-9_]+_kernel(?:<[^>]*>)?")
COUNTS = {"cluster": 7, "greedy": 5, "setcover": 6, "tree": 6, "average": 8, "complete": 8, "cluster_stats": 5, "nj": 7}
ENTRY_OF = {"cluster": ("cluster_init_dev", "cluster_add_hits_dev", "cluster_finish_dev", "cluster_greedy_hits_dev"),
            "greedy": ("cluster_greedy_hits_dev", "cluster_greedy_dev"), "setcover": ("cluster_setcover_hits_dev",),
            "tree": ("cluster_tree_hits_dev",), "average": ("cluster_average_matrix_dev",), "complete": ("cluster_complete_matrix_dev",),
            "cluster_stats": ("cluster_stats_matrix_dev",), "nj": ("nj_matrix_dev",)}


@pytest.fixture(scope="module")
def hg():
    import hypergen_amd
    hypergen_amd.lib()
    return hypergen_amd


def family_of(name):
    m = FAMILIES.fullmatch(name)
    return m.group(1) if m else None


def library_kernels(hg):
    return [n for n in lk.all_kernels(hg.LIB_PATH) if family_of(n)]


def test_census_equals_the_library(hg):
    lib = library_kernels(hg)
    assert len(set(lib)) == len(lib), "two stubs of one spelling"
    names = [r.name for r in cc.ROWS]
    dup = sorted({n for n in names if names.count(n) > 1})
    assert not dup, "rows listed twice: %s" % dup
    for r in cc.ROWS:
        if r.unreachable is not None:
            print("unreachable: %s -- %s" % (r.name, r.unreachable))
    for fam, rows in cc.FAMILY_ROWS.items():
        in_lib = {n for n in lib if family_of(n) == fam}
        listed = {r.name for r in rows}
        assert not sorted(in_lib - listed), "%s instantiations in the library without a census row: %s" % (fam, sorted(in_lib - listed))
        assert not sorted(listed - in_lib), "%s census rows whose kernel the library does not contain: %s" % (fam, sorted(listed - in_lib))
    assert len(lib) == len(names) == 52


def test_census_families_are_complete(hg):
    """the table's own shape: 7 + 5 + 6 + 6 + 8 + 8 + 5 + 7 rows, every row in the list of its family, routed through a
    device-pointer entry point the package binds, its inputs stated"""
    assert set(cc.FAMILY_ROWS) == set(COUNTS)
    for fam, rows in cc.FAMILY_ROWS.items():
        assert len(rows) == COUNTS[fam], fam
        for r in rows:
            assert family_of(r.name) == fam, r
            assert r.entry in ENTRY_OF[fam] and hasattr(hg.lib(), "hg_" + r.entry), r
            assert r.entry.endswith("_dev") and set(r.debug) <= {"pair_limit"} and r.inputs and len(r) == 5, r
    assert sum(COUNTS.values()) == len(cc.ROWS) == 52
    for scheme in ("average", "complete", "nj"):  # the three dense-matrix schemes each have a fill and a mirror
        names = {r.name for r in cc.FAMILY_ROWS[scheme]}
        assert {scheme + "_fill_kernel", scheme + "_mirror_kernel"} <= names
