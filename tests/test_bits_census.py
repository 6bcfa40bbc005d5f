"""The census of bit-level kernels (tests/bits_census.py) against the built library, on the CPU: every binarize, Hamming
popcount, bit-expansion, payload-decoder, 2-bit pack / unpack, run-expansion and synth kernel instantiation `nm -C` lists has
exactly one row, and every row names an instantiation that exists.  (test_gpu_bits_census.py runs the rows.)"""
import re
import subprocess

import pytest

import bits_census as bc

# families, not names: a binarize2_kernel, another hamming_kernel<JN> or a pack2_fast_kernel needs a row too
# (most of them sit in an anonymous namespace, the two bit expansions at file scope: `::name(` or ` name(`)
FAMILIES = re.compile(r"(?:::|(?<=\s))((?:binarize|hamming|expand_bits|expand_runs|hg_hv_unpack|(?:un)?pack2|synth)[a-z0-9_]*_kernel"
                      r"(?:<[^>()]*>)?)\(")


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
    names = [r.name for r in bc.ROWS]
    dup = sorted({n for n in names if names.count(n) > 1})
    assert not dup, "rows listed twice: %s" % dup
    for r in bc.ROWS:
        if r.unreachable is not None:
            print("unreachable: %s -- %s" % (r.name, r.unreachable))
    missing = sorted(lib - set(names))
    stale = sorted(set(names) - lib)
    assert not missing, "instantiations in the library without a census row: %s" % missing
    assert not stale, "census rows whose kernel the library does not contain: %s" % stale


def test_census_families_are_complete():
    """the table's own shape: 3 popcount tiles, 2 bit expansions, 1 row for each of the other seven kernels; the payload
    decoder's row names its four in-kernel routes"""
    assert [r.name for r in bc.HAMMING_ROWS] == ["hamming_kernel<%d>" % jn for jn in (1, 2, 8)]
    assert sorted(r.name for r in bc.EXPAND_ROWS) == ["expand_bits_fp4_kernel", "expand_bits_kernel"]
    assert sorted(r.name for r in bc.OTHER_ROWS) == ["binarize_kernel", "expand_runs_kernel", "hg_hv_unpack_kernel", "pack2_kernel",
                                                     "synth_kernel", "unpack2_kernel", "unpack2_one_kernel"]
    assert len(bc.ROWS) == 12
    unpack, = [r for r in bc.ROWS if r.name == "hg_hv_unpack_kernel"]
    assert set(unpack.inputs) == {(s, l) for s in ("staged", "direct") for l in ("bitpacker8x", "naive")} and len(unpack.inputs) == 4
    for r in bc.ROWS:
        assert r.entry in ("binarize", "hamming", "unpack", "pack2", "unpack2", "stream", "synth"), r
        assert set(r.debug) <= {"ham_path"} and len(r) == 5, r
        assert FAMILIES.fullmatch("::" + r.name + "("), r
