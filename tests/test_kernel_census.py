"""The census of compiled kernels (tests/kernel_census.py) against the built library, on the CPU: every `dist_*kernel` and
`kmer_sample_*<...>` instantiation `nm -C` lists has exactly one row, and every row names an instantiation that exists.
(test_gpu_kernel_census.py runs the rows.)"""
import re
import subprocess

import pytest

import kernel_census as kc

FAMILIES = re.compile(r"::(dist_[a-z0-9_]*kernel(?:<[^>()]*>)?|kmer_sample_(?:shared|long)<[^>()]*>)\(")


@pytest.fixture(scope="module")
def hg():
    import hypergen_amd
    hypergen_amd.lib()
    return hypergen_amd


def library_kernels(hg):
    nm = subprocess.run(["nm", "-C", hg.LIB_PATH], capture_output=True, text=True, check=True).stdout
    return set(FAMILIES.findall(nm))


def test_census_equals_the_library(hg):
    lib = library_kernels(hg)
    names = [r.name for r in kc.ROWS]
    dup = sorted({n for n in names if names.count(n) > 1})
    assert not dup, "rows listed twice: %s" % dup
    reachable = {r.name for r in kc.ROWS if r.unreachable is None}
    for r in kc.ROWS:
        if r.unreachable is not None:
            print("unreachable: %s -- %s" % (r.name, r.unreachable))
    missing = sorted(lib - set(names))
    stale = sorted(set(names) - lib)
    assert not missing, "instantiations in the library without a census row: %s" % missing
    assert not stale, "census rows whose kernel the library does not contain: %s" % stale
    assert reachable <= lib and len(lib) == len(names)


def test_census_families_are_complete(hg):
    """the table's own shape: 28 dist kernels (15 Mash-style with 4 Hamming, 10 containment, 2 small-side, 1 integer) and
    one k-mer kernel per (k, canonical, input form) for k = 1..32, per (k, input form) for k = 33..64 and run-time k"""
    d = [r.name for r in kc.DIST_ROWS]
    assert sum(n.startswith("dist_mfma_kernel<") for n in d) == 15
    assert sum(r.entry == "hamming" and r.name.split(", ")[6] == "true" for r in kc.DIST_ROWS) == 4  # (HAM)
    assert sum(n.startswith("dist_mfma_ctm_kernel<") for n in d) == 10
    assert len(d) == 28 and len(kc.KMER_ROWS) == 128 + 66
    for k in list(range(1, 65)) + list(kc.KMER_LONG_KS):
        for canon in (False, True):
            for packed in (False, True):
                assert kc.kmer_kernel_name(k, canon, packed) in {r.name for r in kc.KMER_ROWS}, (k, canon, packed)
    for r in kc.ROWS:
        assert r.entry in ("dist", "dist_full", "hamming", "kmer"), r
        assert set(r.debug) <= {"dist_path", "dist_tile", "ham_path", "hostfed"}, r
