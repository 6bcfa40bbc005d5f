"""The six census tables together against the built library, on the CPU: the union of their rows is the set of all kernel
instantiations the library holds, every instantiation named exactly once, and no family of kernels split over two tables.
A kernel added to any file without a row in some table fails here, whatever its name; each table's own test says which
family it belongs to."""
import pytest

import bits_census
import cluster_census
import kernel_census
import library_kernels as lk
import min_count_census
import select_census
import set_encode_census

TABLES = {"kernel_census": kernel_census.ROWS, "set_encode_census": set_encode_census.ROWS, "min_count_census": min_count_census.ROWS,
          "bits_census": bits_census.ROWS, "select_census": select_census.ROWS, "cluster_census": cluster_census.ROWS}
# nm leaves these three mangled (a _Float16 * parameter): a listing that drops them must not pass
MANGLED = ("prep_kernel", "prep_fast_kernel", "prep_cen_kernel")


@pytest.fixture(scope="module")
def hg():
    import hypergen_amd
    hypergen_amd.lib()
    return hypergen_amd


def test_tables_cover_the_library_exactly_once(hg):
    lib = lk.all_kernels(hg.LIB_PATH)
    print("%d kernel instantiations in the library, %d census rows in %d tables" % (len(lib), sum(map(len, TABLES.values())), len(TABLES)))
    assert len(set(lib)) == len(lib), "two stubs of one spelling: %s" % sorted({n for n in lib if lib.count(n) > 1})
    for name in MANGLED:
        assert name in lib, "the listing lost %s" % name
    where = {}
    for table, rows in TABLES.items():
        for r in rows:
            where.setdefault(r.name, []).append(table)
    twice = {n: t for n, t in where.items() if len(t) > 1}
    assert not twice, "kernels named more than once: %s" % twice
    missing = sorted(set(lib) - set(where))
    stale = sorted(set(where) - set(lib))
    assert not missing, "instantiations in the library that no census table names: %s" % missing
    assert not stale, "census rows whose kernel the library does not contain: %s" % {n: where[n] for n in stale}
    assert len(lib) == len(where) == sum(map(len, TABLES.values()))


def test_no_family_is_split_over_two_tables():
    tables_of = {}
    for table, rows in TABLES.items():
        for r in rows:
            tables_of.setdefault(lk.family(r.name), set()).add(table)
    split = {f: sorted(t) for f, t in tables_of.items() if len(t) > 1}
    assert not split, "families that appear in two tables: %s" % split
