"""libhypergen_tri.so and `hyper-gen triangle`, the parts that need no GPU: include/hypergen_tri.h, the library's exports and the
Python mirror agree; the library borrows nothing from the test oracle and links the main one; hg_tri_text_bytes and
hg_tri_field_offset against tests/tri_ref.py at the smallest sets, across a block boundary and where 8 i (i - 1) / 2 passes
2^33 and 2^35; the reference itself by hand; the command line describes the subcommand under `triangle --help` only, leaves the
general help and the usage line as they were, and rejects what it must before a device is opened."""
import os
import re
import subprocess

import numpy as np
import pytest

import tri_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "hypergen_tri.h")
LAYOUTS = (tri_ref.LOWER, tri_ref.FULL)


@pytest.fixture(scope="module")
def hg():
    import hypergen_amd
    hypergen_amd.lib_tri()
    return hypergen_amd


def exported(path):
    nm = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return [line.split()[-1] for line in nm.splitlines() if line.split()[-2] in ("T", "t", "W")]


def test_every_declared_symbol_is_exported_and_bound(hg):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(hg_tri_\w+|hg_tri)\s*\(", text)))
    assert declared == sorted(hg.TRI_EXPORTS) and len(declared) == 11
    c_names = sorted(s for s in exported(hg.TRI_LIB_PATH) if s.startswith("hg_tri") and not s.startswith("_Z"))
    assert c_names == declared
    for name in declared:
        assert getattr(hg.lib_tri(), name).argtypes is not None, name
    # the other libraries' surfaces are what they were: nothing of this one went into them
    hg.lib_aa(), hg.lib_tx(), hg.lib_rec(), hg.lib_frag(), hg.lib_hist()
    assert not [s for s in hg.EXPORTS + hg.AA_EXPORTS + hg.TX_EXPORTS + hg.REC_EXPORTS + hg.FRAG_EXPORTS + hg.HIST_EXPORTS if s.startswith("hg_tri")]
    for path in (hg.LIB_PATH, hg.AA_LIB_PATH, hg.TX_LIB_PATH, hg.REC_LIB_PATH, hg.FRAG_LIB_PATH, hg.HIST_LIB_PATH):
        assert not [s for s in exported(path) if "hg_tri" in s]


def test_library_defines_no_oracle_symbol_and_links_the_main_library(hg):
    assert not [s for s in exported(hg.TRI_LIB_PATH) if "orc_" in s]
    dyn = subprocess.run(["readelf", "-d", hg.TRI_LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "libhypergen_hip.so" in dyn and "$ORIGIN" in dyn


def test_constants_and_geometry(hg):
    assert (hg.TRI_LOWER, hg.TRI_FULL, hg.TRI_FIELD_BYTES) == (tri_ref.LOWER, tri_ref.FULL, tri_ref.FIELD)
    src = open(HEADER).read()
    assert "#define HG_TRI_LOWER 0u" in src and "#define HG_TRI_FULL 1u" in src and "#define HG_TRI_FIELD_BYTES 8u" in src
    geo = hg.tri_geometry()
    assert geo["threads"] == 256 and geo["tile_cols"] == geo["threads"] and geo["tile_rows"] >= 2
    assert len(hg.tri_kernel_names()) == len(set(hg.tri_kernel_names())) == 1


# ---- sizes and offsets -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [0, 1, 2, 3])
def test_sizes_and_offsets_of_the_smallest_sets(hg, n):
    for layout in LAYOUTS:
        assert hg.tri_text_bytes(layout, 0, n, n) == tri_ref.text_bytes(layout, 0, n, n) == 8 * (n * n if layout == tri_ref.FULL else n * (n - 1) // 2)
        for row0 in range(n + 1):
            for rows in range(n - row0 + 1):
                assert hg.tri_text_bytes(layout, row0, rows, n) == tri_ref.text_bytes(layout, row0, rows, n)
            for i in range(row0, n):
                for j in range(i if layout == tri_ref.LOWER else n):
                    assert hg.tri_field_offset(layout, row0, i, j, n) == tri_ref.field_offset(layout, row0, i, j, n)
    # by hand: three sketches, LOWER: (1, 0) at 0, (2, 0) at 8, (2, 1) at 16
    if n == 3:
        assert [hg.tri_field_offset(tri_ref.LOWER, 0, i, j, 3) for i, j in ((1, 0), (2, 0), (2, 1))] == [0, 8, 16]
        assert [hg.tri_field_offset(tri_ref.FULL, 0, i, j, 3) for i, j in ((0, 0), (0, 2), (1, 0), (2, 2))] == [0, 16, 24, 64]
        assert hg.tri_field_offset(tri_ref.LOWER, 2, 2, 1, 3) == 8 and hg.tri_field_offset(tri_ref.FULL, 2, 2, 1, 3) == 8


def test_blocks_tile_the_text_across_a_block_boundary(hg):
    n, rb = 1000, 37
    for layout in LAYOUTS:
        at = 0
        for row0 in range(0, n, rb):
            rows = min(rb, n - row0)
            assert hg.tri_field_offset(layout, 0, row0, 0, n) == at == tri_ref.field_offset(layout, 0, row0, 0, n)
            # the last field of the block's last row ends the block; the next block's first field follows it
            i = row0 + rows - 1
            last_j = (i - 1 if layout == tri_ref.LOWER else n - 1)
            size = hg.tri_text_bytes(layout, row0, rows, n)
            assert size == tri_ref.text_bytes(layout, row0, rows, n)
            if size:
                assert hg.tri_field_offset(layout, row0, i, max(last_j, 0), n) + (8 if last_j >= 0 else 0) == size
            assert hg.tri_field_offset(layout, row0, i + 1, 0, n) == size  # (the row behind the block starts where the block ends)
            at += size
        assert at == hg.tri_text_bytes(layout, 0, n, n)


@pytest.mark.parametrize("i,bit", [(46_341, 33), (92_682, 35)])
def test_offsets_are_64_bit(hg, i, bit):
    """the text passes 2^33 bytes inside row 46 341 and 2^35 inside row 92 682: the row starts below the power, the next one above"""
    assert 8 * tri_ref.tri(i) < 2 ** bit <= 8 * tri_ref.tri(i + 1)
    for k in (i - 1, i, i + 1):
        want = 8 * (k * (k - 1) // 2)
        assert hg.tri_field_offset(tri_ref.LOWER, 0, k, 0, k + 5) == tri_ref.field_offset(tri_ref.LOWER, 0, k, 0, k + 5) == want
        assert hg.tri_field_offset(tri_ref.LOWER, 0, k, k - 1, k + 5) == want + 8 * (k - 1)
        assert hg.tri_text_bytes(tri_ref.LOWER, 0, k, k) == want
        assert hg.tri_text_bytes(tri_ref.LOWER, k - 3, 3, k) == 8 * (3 * k - 9) + 8 * 3  # rows k - 3, k - 2, k - 1
        assert hg.tri_field_offset(tri_ref.LOWER, k - 3, k, 7, k + 5) == 8 * (3 * k - 6) + 56
        assert hg.tri_text_bytes(tri_ref.FULL, 0, k, k) == tri_ref.text_bytes(tri_ref.FULL, 0, k, k) == 8 * k * k
        assert hg.tri_field_offset(tri_ref.FULL, 5, k, k - 1, k) == 8 * ((k - 5) * k + k - 1)
    top = 2 ** 31 - 1
    assert hg.tri_text_bytes(tri_ref.LOWER, 0, top, top) == 8 * (top * (top - 1) // 2) < 2 ** 64
    assert hg.tri_text_bytes(2, 0, 5, 5) == 0 and hg.tri_field_offset(2, 0, 3, 1, 5) == 0  # an unknown layout


# ---- the reference itself, by hand -------------------------------------------------------------------------------------------------

def test_reference_rules_by_hand():
    nan, inf = float("nan"), float("inf")
    values = [nan, -1.0, -0.0, inf, -inf, 0.0004, 100.0001, 101.0, 94.999, 95.0, 9.5]
    assert tri_ref.milli(values).tolist() == [0, 0, 0, 100_000, 0, 0, 100_000, 100_000, 94_999, 95_000, 9_500]
    assert tri_ref.field(0) == b"  0.000\t" and tri_ref.field(95_123, True) == b" 95.123\n" and tri_ref.field(100_000) == b"100.000\t"
    assert tri_ref.field(9_005) == b"  9.005\t" and tri_ref.field(10_000) == b" 10.000\t"
    with pytest.raises(tri_ref.Invalid):
        tri_ref.field(100_001)
    a = np.array([[1, 2, 3], [4, 5, 6], [7, 8, 9]], np.float32)
    assert tri_ref.block_text(a, tri_ref.FULL) == b"  1.000\t  2.000\t  3.000\n  4.000\t  5.000\t  6.000\n  7.000\t  8.000\t  9.000\n"
    assert tri_ref.block_text(a, tri_ref.LOWER) == b"  4.000\n  7.000\t  8.000\n"
    assert tri_ref.block_text(a[:2], tri_ref.LOWER, 2) == b"  1.000\t  2.000\n  4.000\t  5.000\t  6.000\n"  # rows 2 and 3
    assert tri_ref.block_text(a[:1], tri_ref.LOWER, 0) == b""
    with pytest.raises(tri_ref.Invalid):
        tri_ref.block_text(a, tri_ref.LOWER, 2)  # row 4 would need four columns
    # every m through the vector formatter and the scalar one
    m = np.arange(100_001, dtype=np.int64).reshape(1, -1)
    f = tri_ref.fields_of_milli(m)
    for k in (0, 9, 10, 99, 100, 999, 1000, 9_999, 10_000, 95_123, 99_999, 100_000):
        assert f[0, k].tobytes() == tri_ref.field(k)
    assert len(tri_ref.block_text(np.zeros((5, 7), np.float32), tri_ref.LOWER, 3)) == tri_ref.text_bytes(tri_ref.LOWER, 3, 5, 7)


def test_reference_file_by_hand():
    m = [[100_000, 1, 2], [95_123, 100_000, 3], [0, 7, 100_000]]
    names = [b"a", b"b c", b"d"]
    assert tri_ref.file_text(names, m, tri_ref.LOWER) == b"3\na\nb c\t 95.123\nd\t  0.000\t  0.007\n"
    assert tri_ref.file_text(names, m, tri_ref.FULL) == (b"3\na\t100.000\t  0.001\t  0.002\nb c\t 95.123\t100.000\t  0.003\n"
                                                          b"d\t  0.000\t  0.007\t100.000\n")
    assert tri_ref.file_text([b"only"], [[100_000]], tri_ref.LOWER) == b"1\nonly\n"
    assert tri_ref.file_text([b"only"], [[100_000]], tri_ref.FULL) == b"1\nonly\t100.000\n"
    assert tri_ref.file_text([], [], tri_ref.LOWER) == b"0\n" == tri_ref.file_text([], [], tri_ref.FULL)
    # from dist's TSV: i < j once under a symmetric metric, every i != j under containment
    tsv = b"a\tb c\t95.123\na\td\t0.000\nb c\td\t0.007\n"
    assert tri_ref.file_from_tsv(names, tsv, tri_ref.LOWER) == tri_ref.file_text(names, m, tri_ref.LOWER)
    tsv = b"a\tb c\t0.001\na\td\t0.002\nb c\ta\t95.123\nb c\td\t0.003\nd\ta\t0.000\nd\tb c\t0.007\n"
    assert tri_ref.file_from_tsv(names, tsv, tri_ref.FULL) == tri_ref.file_text(names, m, tri_ref.FULL)
    with pytest.raises(tri_ref.Invalid):
        tri_ref.file_from_tsv(names, b"a\tb c\t95.123\n", tri_ref.LOWER)  # pairs are missing
    with pytest.raises(tri_ref.Invalid):
        tri_ref.file_from_tsv(names, tsv + b"a\td\t0.002\n", tri_ref.FULL)  # a pair twice


# ---- command line ------------------------------------------------------------------------------------------------------------

def run_cli(hg, *args, cwd=None):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")  # (no device: all of this is decided before one is opened)
    return subprocess.run([hg.CLI_PATH, *args], capture_output=True, text=True, env=env, cwd=cwd)


def test_the_paragraph_appears_under_triangle_help_only(hg):
    general = run_cli(hg, "--help")
    assert general.returncode == 0 and "triangle" not in general.stdout
    assert "hyper-gen cluster -p {sketch_file} -o {output_clusters}" in general.stdout
    tr = run_cli(hg, "triangle", "--help")
    assert tr.returncode == 0 and tr.stdout.startswith(general.stdout) and tr.stderr == ""
    assert run_cli(hg, "triangle", "-h").stdout == tr.stdout
    tail = tr.stdout[len(general.stdout):]
    assert tail.startswith("hyper-gen triangle -p {sketch_file} -o {output_matrix} [-t N] [--ani_metric mash|max_containment|containment]:")
    assert '("  0.000", " 95.123", "100.000")' in tail  # (the padding as it is written)
    para = " ".join(tail.split())
    for word in ("PHYLIP-like", "first visible GPU", "The first line is n", "its name as dist writes it", "A field is 8 bytes",
                 "right-aligned in 7 characters", '" 95.123", "100.000"', "then a tab, or a newline behind the row's last field",
                 "lower triangle", "row 0 its name alone", "8 * i * (i - 1) / 2", "writes the square", "8 * i * n", "plus 8 * j",
                 "a reader can seek to any pair", "can be reproduced from dist -a 0", "-a is accepted and ignored", "-t threads [16]"):
        assert word in para, word
    for mode in ("sketch", "dist", "search", "cluster"):
        assert "triangle" not in run_cli(hg, mode, "--help").stdout


def test_triangle_is_the_fifth_mode_bit():
    src = open(os.path.join(ROOT, "hyper-gen_amd", "csrc", "hg_cli.cpp")).read()
    assert "enum : unsigned { SKETCH = 1, DIST = 2, SEARCH = 4, CLUSTER = 8, TRIANGLE = 16, ANY = 31 };" in src
    table = src[src.index("const Option options[] = {"):src.index("const size_t N_OPTIONS")]
    assert "TRIANGLE" not in table and len(re.findall(r"^\s*\{\"", table, flags=re.M)) == 42  # no option row names it, none was added


REQUIRED = "error: the following required arguments were not provided: --path --out\n"
CLI_ERRORS = [
    (("triangle",), REQUIRED),
    (("triangle", "-p", "x.sketch"), REQUIRED),
    (("triangle", "-o", "x.phy"), REQUIRED),
    (("triangle", "-o", "x.phy", "-a", "3", "-t", "4", "--ani_metric", "containment"), REQUIRED),  # (-a is accepted)
    (("triangle", "--shards", "2"), "error: --shards is not supported by triangle: it runs on the first visible GPU\n"),
    (("triangle", "--histogram", "f"), "error: --histogram is not supported by triangle: it counts the ANI values of dist's comparison\n"),
    (("triangle", "--linkage", "greedy"), "error: --linkage is not supported by triangle: it chooses how cluster forms its clusters\n"),
    (("triangle", "--pairs", "f"), "error: --pairs is not supported by triangle: it names the pairs dist evaluates\n"),
    (("triangle", "--newick", "f"), "error: --newick is not supported by triangle: it draws the tree of dist's comparison\n"),
    (("triangle", "--stats", "f"), "error: --stats is not supported by triangle: it describes the clusters of cluster\n"),
    (("triangle", "--ani_metric", "jaccard"), "error: invalid value 'jaccard' for '--ani_metric' (mash | containment | max_containment)\n"),
    (("triangle", "--frobnicate"), "error: unexpected argument '--frobnicate'\n"),
    (("triangles",), "error: unknown subcommand 'triangles'\n"),
    ((), "error: usage: hyper-gen <sketch|dist|search|cluster> [options]   (see --help)\n"),
]


@pytest.mark.parametrize("args,stderr", CLI_ERRORS)
def test_cli_error_lines(hg, args, stderr, tmp_path):
    r = run_cli(hg, *args, cwd=str(tmp_path))
    assert (r.returncode, r.stdout, r.stderr) == (2, "", stderr)
    assert os.listdir(str(tmp_path)) == []  # nothing was written
