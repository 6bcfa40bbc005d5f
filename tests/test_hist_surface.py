"""libhypergen_hist.so and `hyper-gen dist --histogram`, the parts that need no GPU: include/hypergen_hist.h, the library's
exports and the Python mirror agree; the library borrows nothing from the test oracle and links the main one; hg_hist_bins at
the ends of its range; the reference of tests/hist_ref.py by hand -- clamps, rounding, a bin edge, the three selections, the
file; the command line describes the options in `dist --help` only and rejects what it must before a device is opened."""
import os
import re
import subprocess

import numpy as np
import pytest

import hist_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "hypergen_hist.h")


@pytest.fixture(scope="module")
def hg():
    import hypergen_amd
    hypergen_amd.lib_hist()
    return hypergen_amd


def exported(path):
    nm = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return [line.split()[-1] for line in nm.splitlines() if line.split()[-2] in ("T", "t", "W")]


def test_every_declared_symbol_is_exported_and_bound(hg):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(hg_hist_\w+|hg_hist)\s*\(", text)))
    assert declared == sorted(hg.HIST_EXPORTS) and len(declared) == 10
    c_names = sorted(s for s in exported(hg.HIST_LIB_PATH) if s.startswith("hg_hist") and not s.startswith("_Z"))
    assert c_names == declared
    for name in declared:
        assert getattr(hg.lib_hist(), name).argtypes is not None, name
    # the other libraries' surfaces are what they were: nothing of this one went into them
    hg.lib_aa(), hg.lib_tx(), hg.lib_rec(), hg.lib_frag()
    assert not [s for s in hg.EXPORTS + hg.AA_EXPORTS + hg.TX_EXPORTS + hg.REC_EXPORTS + hg.FRAG_EXPORTS if s.startswith("hg_hist")]
    for path in (hg.LIB_PATH, hg.AA_LIB_PATH, hg.TX_LIB_PATH, hg.REC_LIB_PATH, hg.FRAG_LIB_PATH):
        assert not [s for s in exported(path) if "hg_hist" in s]


def test_library_defines_no_oracle_symbol_and_links_the_main_library(hg):
    assert not [s for s in exported(hg.HIST_LIB_PATH) if "orc_" in s]
    dyn = subprocess.run(["readelf", "-d", hg.HIST_LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "libhypergen_hip.so" in dyn and "$ORIGIN" in dyn


def test_bins_and_geometry(hg):
    want = {0: 0, 1: 100_001, 3: 33_334, 100: 1001, 99_999: 2, 100_000: 2, 100_001: 0}
    assert {w: hg.hist_bins(w) for w in want} == want
    assert {w: hist_ref.bins(w) for w in want} == want
    assert hg.hist_bins(0xFFFFFFFF) == 0 and hg.hist_bins(50_000) == 3 and hg.hist_bins(50_001) == 2
    assert (hg.HIST_ALL, hg.HIST_UPPER, hg.HIST_OFFDIAG, hg.HIST_MILLI_MAX) == (hist_ref.ALL, hist_ref.UPPER, hist_ref.OFFDIAG, hist_ref.MILLI_MAX)
    geo = hg.hist_geometry()
    assert geo["threads"] == 256 and geo["tile_cols"] == geo["threads"] and geo["tile_rows"] >= 2
    assert geo["lds_bins"] * 4 <= 64 * 1024 and geo["lds_bins"] >= 1001 * 4  # several workgroups per CU; the default width keeps four copies
    assert geo["tile_rows"] * geo["tile_cols"] < 2 ** 32                      # an LDS counter holds a tile
    assert len(hg.hist_kernel_names()) == len(set(hg.hist_kernel_names())) == 1


# ---- the reference itself, by hand ---------------------------------------------------------------------------------------------

def test_reference_rules_by_hand():
    nan, inf = float("nan"), float("inf")
    values = [nan, -1.0, -0.0, inf, 0.0004, 100.0004, 100.5, 94.999, 95.0, 95.001]
    assert hist_ref.milli(values).tolist() == [0, 0, 0, 100_000, 0, 100_000, 100_000, 94_999, 95_000, 95_001]
    c = hist_ref.counts(np.array([values], np.float32), 100)
    assert c.size == 1001 and {int(b): int(c[b]) for b in np.flatnonzero(c)} == {0: 4, 949: 1, 950: 2, 1000: 3}
    c = hist_ref.counts(np.array([values], np.float32), 1)
    assert c.size == 100_001 and {int(b): int(c[b]) for b in np.flatnonzero(c)} == {0: 4, 94_999: 1, 95_000: 1, 95_001: 1, 100_000: 3}
    c = hist_ref.counts(np.array([values], np.float32), 100_000)
    assert c.tolist() == [7, 3]
    c = hist_ref.counts(np.array([values], np.float32), 33_333)  # bins [0, 33 332], [33 333, 66 665], [66 666, 99 998], [99 999, 100 000]
    assert c.tolist() == [4, 0, 3, 3]
    with pytest.raises(hist_ref.Invalid):
        hist_ref.counts(np.zeros((1, 1), np.float32), 0)
    with pytest.raises(hist_ref.Invalid):
        hist_ref.counts(np.zeros((1, 1), np.float32), 100_001)


def test_reference_selections_by_hand():
    a = np.array([[10, 20, 30], [40, 50, 60], [70, 80, 90]], np.float32)

    def bins_hit(pairs, row0=0, col0=0):
        return sorted(int(b) for b in np.repeat(np.arange(11), hist_ref.counts(a, 10_000, pairs, row0, col0).astype(np.int64)))

    assert bins_hit(hist_ref.ALL) == [1, 2, 3, 4, 5, 6, 7, 8, 9]
    assert bins_hit(hist_ref.UPPER) == [2, 3, 6] and bins_hit(hist_ref.OFFDIAG) == [2, 3, 4, 6, 7, 8]
    # the block at rows 5.., columns 6..: the diagonal runs through (1, 0) and (2, 1)
    assert bins_hit(hist_ref.UPPER, 5, 6) == [1, 2, 3, 5, 6, 9] and bins_hit(hist_ref.OFFDIAG, 5, 6) == [1, 2, 3, 5, 6, 7, 9]
    assert bins_hit(hist_ref.UPPER, 9, 0) == [] and bins_hit(hist_ref.UPPER, 0, 9) == [1, 2, 3, 4, 5, 6, 7, 8, 9]
    assert hist_ref.selected(2, 2, 2 ** 31 - 2, 2 ** 31 - 2, hist_ref.UPPER).tolist() == [[False, True], [False, False]]
    with pytest.raises(hist_ref.Invalid):
        hist_ref.counts(a, 100, 3)


def test_reference_file_and_width_by_hand():
    assert hist_ref.file_text([5, 0, 2], 50_000) == "0.000\t49.999\t5\t7\n50.000\t99.999\t0\t2\n100.000\t100.000\t2\t2\n"
    assert hist_ref.file_text([1, 2 ** 40], 100_000) == "0.000\t99.999\t1\t%d\n100.000\t100.000\t%d\t%d\n" % (2 ** 40 + 1, 2 ** 40, 2 ** 40)
    text = hist_ref.file_text(np.zeros(1001, np.uint64), 100)
    assert text.count("\n") == 1001 and text.splitlines()[950] == "95.000\t95.099\t0\t0" and text.splitlines()[-1] == "100.000\t100.000\t0\t0"
    good = {"0.1": 100, "1": 1000, "0.001": 1, "100": 100_000, "100.000": 100_000, ".5": 500, "2.": 2000, "00.25": 250}
    assert {t: hist_ref.parse_bin(t) for t in good} == good
    for bad in ("0", "0.0001", "100.001", "abc", "", ".", "1e1", "-1", "+1", " 1", "1.0000", "0.000", "1000000000000000000000"):
        with pytest.raises(hist_ref.Invalid):
            hist_ref.parse_bin(bad)
    tsv = "a\tb\t95.000\nc d\te\t0.007\nf\tg\t100.000\n"
    assert hist_ref.tsv_milli(tsv).tolist() == [95_000, 7, 100_000]
    assert hist_ref.counts_of_milli(hist_ref.tsv_milli(tsv), 50_000).tolist() == [1, 1, 1]


# ---- command line ------------------------------------------------------------------------------------------------------------

def run_cli(hg, *args, cwd=None):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")  # (no device: all of this is decided before one is opened)
    return subprocess.run([hg.CLI_PATH, *args], capture_output=True, text=True, env=env, cwd=cwd)


def test_help_texts_name_the_options_and_the_general_help_does_not(hg):
    general = run_cli(hg, "--help")
    assert general.returncode == 0 and "--histogram" not in general.stdout
    di = run_cli(hg, "dist", "--help")
    assert di.returncode == 0 and di.stdout.startswith(general.stdout)
    tail = di.stdout[len(general.stdout):]
    at = tail.index("\ndist --histogram FILE [--histogram_bin B]:")
    assert at > tail.index("\ndist --fragments [--fragment_ani T]") and "--histogram" not in tail[:at]
    para = " ".join(tail[at:].split())
    for word in ("--histogram_bin B [0.1]", "0.001 to 100", "at most three decimals", "1001 bins", "whatever -a is", "i < j", "i != j",
                 "as dist prints it", "in all higher bins", "PRINT at least", "it is not the number of lines dist -a x writes",
                 "94.9996 prints 95.000 and fails -a 95", "second pass", "first visible GPU", "once per 8192 bins",
                 "-o is what it is without --histogram", "goes with --columns and --newick", "--pairs, --fragments or --shards"):
        assert word in para, word
    for mode in ("sketch", "search", "cluster"):
        assert "--histogram" not in run_cli(hg, mode, "--help").stdout


def test_the_two_options_are_rows_of_the_option_table_which_stays_within_the_width_of_given():
    src = open(os.path.join(ROOT, "hyper-gen_amd", "csrc", "hg_cli.cpp")).read()
    table = src[src.index("const Option options[] = {"):src.index("const size_t N_OPTIONS")]
    rows = re.findall(r"^    \{\"([a-z_]+)\",", table, flags=re.M)  # every row, whatever follows its name on the line
    width, = map(int, re.findall(r"std::bitset<(\d+)> given;", src))  # Cli::given, a bit per row
    assert rows[-2:] == ["histogram", "histogram_bin"] and len(rows) == len(set(rows)) == 42 <= width
    assert len(re.findall(r"^\s*\{\"", table, flags=re.M)) == 42  # no row hides from the count above behind another indentation
    assert "static_assert(N_OPTIONS <= decltype(Cli::given)().size()" in src


BAD_BIN = " (the width of a bin as an ANI: above 0, at most 100, at most three decimals)\n"
NOT_DIST = ": it counts the ANI values of dist's comparison\n"
CLI_ERRORS = [
    # the width
    (("dist", "--histogram", "h.tsv", "--histogram_bin", "0"), "error: invalid value '0' for '--histogram_bin'" + BAD_BIN),
    (("dist", "--histogram", "h.tsv", "--histogram_bin", "0.0001"), "error: invalid value '0.0001' for '--histogram_bin'" + BAD_BIN),
    (("dist", "--histogram_bin=100.001", "--histogram", "h.tsv"), "error: invalid value '100.001' for '--histogram_bin'" + BAD_BIN),
    (("dist", "--histogram", "h.tsv", "--histogram_bin", "abc"), "error: invalid value 'abc' for '--histogram_bin'" + BAD_BIN),
    (("dist", "--histogram", "h.tsv", "--histogram_bin", ""), "error: invalid value '' for '--histogram_bin'" + BAD_BIN),
    (("dist", "--histogram", "h.tsv", "--histogram_bin="), "error: invalid value '' for '--histogram_bin'" + BAD_BIN),
    (("dist", "--histogram", "h.tsv", "--histogram_bin", "1e1"), "error: invalid value '1e1' for '--histogram_bin'" + BAD_BIN),
    (("dist", "--histogram", "h.tsv", "--histogram_bin", "-1"), "error: invalid value '-1' for '--histogram_bin'" + BAD_BIN),
    (("dist", "--histogram", "h.tsv", "--histogram_bin"), "error: a value is required for '--histogram_bin'\n"),
    (("dist", "--histogram", ""), "error: invalid value '' for '--histogram' (a file name)\n"),
    (("dist", "--histogram"), "error: a value is required for '--histogram'\n"),
    # the subcommands that do not take them
    (("sketch", "--histogram", "h.tsv"), "error: --histogram is not supported by sketch" + NOT_DIST),
    (("search", "--histogram=h.tsv"), "error: --histogram is not supported by search" + NOT_DIST),
    (("cluster", "--histogram", "h.tsv"), "error: --histogram is not supported by cluster" + NOT_DIST),
    (("sketch", "--histogram_bin", "1"), "error: --histogram_bin is not supported by sketch: it belongs to dist --histogram\n"),
    (("search", "--histogram_bin", "1"), "error: --histogram_bin is not supported by search: it belongs to dist --histogram\n"),
    (("cluster", "--histogram_bin", "1"), "error: --histogram_bin is not supported by cluster: it belongs to dist --histogram\n"),
    # what it does not go with
    (("dist", "--histogram", "h.tsv", "--shards", "2"),
     "error: --histogram is not supported with --shards: dist with --histogram runs on the first visible GPU\n"),
    (("dist", "--pairs", "p.tsv", "--histogram", "h.tsv"),
     "error: --histogram is not supported with --pairs: it counts every pair of the comparison, not the listed ones\n"),
    (("dist", "--histogram", "h.tsv", "--fragments"),
     "error: --histogram is not supported with --fragments: it counts the ANI of whole sketches, not of fragments\n"),
    (("dist", "--histogram_bin", "1"), "error: --histogram_bin needs --histogram: without it dist counts no pairs\n"),
    # what is not rejected goes on to the required arguments, as ever
    (("dist", "--histogram", "h.tsv"), "error: the following required arguments were not provided: --path_r --path_q --out\n"),
    (("dist", "--histogram=h.tsv", "--histogram_bin=0.001", "--columns", "mash", "--newick", "t.nwk", "--ani_metric", "max_containment"),
     "error: the following required arguments were not provided: --path_r --path_q --out\n"),
    (("dist", "--histogram", "h.tsv", "--histogram_bin", "100", "--shards", "0"),
     "error: the following required arguments were not provided: --path_r --path_q --out\n"),
]


@pytest.mark.parametrize("args,stderr", CLI_ERRORS)
def test_cli_error_lines(hg, args, stderr, tmp_path):
    r = run_cli(hg, *args, cwd=str(tmp_path))
    assert (r.returncode, r.stdout, r.stderr) == (2, "", stderr)
    assert os.listdir(str(tmp_path)) == []  # nothing was written
