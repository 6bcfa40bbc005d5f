"""libhypergen_frag.so, `hyper-gen sketch --fragment` and `hyper-gen dist --fragments`, the parts that need no GPU:
include/hypergen_frag.h, the library's exports and the Python mirror agree; the library borrows nothing from the test oracle
and links the main one; hg_frag_plan against tests/frag_ref.py at every length where the plan changes; the reference's own
tie, clamp and rounding rules by hand; the command line describes the options in `sketch --help` and `dist --help` only and
rejects what it must before a device is opened."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import frag_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "hypergen_frag.h")


@pytest.fixture(scope="module")
def hg():
    import hypergen_amd
    hypergen_amd.lib_frag()
    return hypergen_amd


def exported(path):
    nm = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return [line.split()[-1] for line in nm.splitlines() if line.split()[-2] in ("T", "t", "W")]


def test_every_declared_symbol_is_exported_and_bound(hg):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(hg_frag_\w+)\s*\(", text)))
    assert declared == sorted(hg.FRAG_EXPORTS) and len(declared) == 11
    c_names = sorted(s for s in exported(hg.FRAG_LIB_PATH) if s.startswith("hg_frag_") and not s.startswith("_Z"))
    assert c_names == declared
    for name in declared:
        assert getattr(hg.lib_frag(), name).argtypes is not None, name
    # the other libraries' surfaces are what they were: nothing of this one went into them
    hg.lib_aa(), hg.lib_tx(), hg.lib_rec()
    assert not [s for s in hg.EXPORTS + hg.AA_EXPORTS + hg.TX_EXPORTS + hg.REC_EXPORTS if s.startswith("hg_frag_")]
    for path in (hg.LIB_PATH, hg.AA_LIB_PATH, hg.TX_LIB_PATH, hg.REC_LIB_PATH):
        assert not [s for s in exported(path) if "hg_frag_" in s]


def test_library_defines_no_oracle_symbol_and_links_the_main_library(hg):
    assert not [s for s in exported(hg.FRAG_LIB_PATH) if "orc_" in s]
    dyn = subprocess.run(["readelf", "-d", hg.FRAG_LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "libhypergen_hip.so" in dyn and "$ORIGIN" in dyn


def test_records_and_geometry(hg):
    assert hg.FRAG_PAIR_DTYPE == frag_ref.PAIR_DTYPE and hg.FRAG_PAIR_DTYPE.itemsize == 16
    assert hg.FRAG_BEST_DTYPE == frag_ref.BEST_DTYPE and hg.FRAG_BEST_DTYPE.itemsize == 8
    assert hg.FRAG_NONE == frag_ref.NONE
    geo = hg.frag_geometry()
    assert geo["wave"] == 64 and geo["col_tile"] % geo["wave"] == 0 and geo["fold_threads"] % geo["wave"] == 0 and geo["row_chunk"] >= 2
    assert len(hg.frag_kernel_names()) == len(set(hg.frag_kernel_names())) == 2


# ---- the window plan ---------------------------------------------------------------------------------------------------------

def plan_lengths(W, S):
    return [0, 1, W - 1, W, W + 1, W + S - 1, W + S, W + S + 1, 10 * W + W // 2 - 1, 10 * W + W // 2]


@pytest.mark.parametrize("W,S", [(1000, 1000), (1000, 500), (4, 4), (4000, 2000), (2000, 2000), (64, 12)])
def test_plan_equals_the_reference(hg, W, S):
    for length in plan_lengths(W, S):
        want = frag_ref.plan(length, W, S)
        st, n, starts, lens = hg.frag_plan(length, W, S)
        assert (st, n) == (hg.OK, len(want)), (length, W, S)
        assert list(zip(starts.tolist(), lens.tolist())) == want, (length, W, S)
        # the formula of the header, with the dropped tail
        full = 1 if length <= W else 1 + -(-(length - W) // S)
        assert n in (full, full - 1) and (n == full or 2 * (length - (full - 1) * S) < W)
        assert starts.tolist() == [j * S for j in range(n)] and all(0 < x <= W for x in lens.tolist()[: n - 1])
        if S * 2 <= W or length <= W:
            assert n == full  # nothing is dropped
        assert length == 0 or int(starts[-1] + lens[-1]) <= length
        assert length <= W or int(starts[-1] + lens[-1]) == length or S == W  # only disjoint windows leave a tail out


def test_plan_by_hand(hg):
    assert frag_ref.plan(0, 1000, 1000) == [(0, 0)] and frag_ref.plan(999, 1000, 500) == [(0, 999)]
    assert frag_ref.plan(1499, 1000, 1000) == [(0, 1000)]                  # a tail of 499 < 500 is dropped
    assert frag_ref.plan(1500, 1000, 1000) == [(0, 1000), (1000, 500)]     # one of 500 stays
    assert frag_ref.plan(1001, 1000, 500) == [(0, 1000), (500, 501)]
    assert frag_ref.plan(2000, 1000, 500) == [(0, 1000), (500, 1000), (1000, 1000)]
    assert frag_ref.plan(2001, 1000, 500) == [(0, 1000), (500, 1000), (1000, 1000), (1500, 501)]


def test_plan_refusals_and_capacity(hg):
    for W, S in ((1000, 0), (1000, 1004), (1002, 500), (1000, 502), (0, 0), (8, 2), (1000, 1)):
        st, n, _, _ = hg.frag_plan(5000, W, S)
        assert (st, n) == (hg.ERR_INVALID, 0), (W, S)
        with pytest.raises(frag_ref.Invalid):
            frag_ref.plan(5000, W, S)
    want = frag_ref.plan(10_499, 1000, 500)
    st, n, starts, lens = hg.frag_plan(10_499, 1000, 500, cap=3)
    assert (st, n) == (hg.ERR_CAPACITY, len(want)) and list(zip(starts.tolist(), lens.tolist())) == want[:3]
    st, n, _, _ = hg.frag_plan(10_499, 1000, 500, cap=0)
    assert (st, n) == (hg.ERR_CAPACITY, len(want))
    assert hg.lib_frag().hg_frag_plan(100, 1000, 1000, None, None, 0, None) == hg.ERR_INVALID
    n_out = C.c_size_t(0)
    assert hg.lib_frag().hg_frag_plan(100, 1000, 1000, None, None, 1, C.byref(n_out)) == hg.ERR_INVALID  # room, but nowhere to write


# ---- the reference itself, by hand ---------------------------------------------------------------------------------------------

def test_reference_rules_by_hand():
    nan = float("nan")
    assert frag_ref.milli([nan, -1.0, 100.0004, 100.5, 0.0, 99.9994, 95.0625, 95.1875]).tolist() == [0, 0, 100000, 100000, 0, 99999, 95062, 95188]
    assert frag_ref.threshold(90) == 90000 and frag_ref.threshold(nan) == 0 and frag_ref.threshold(250) == 100000
    ani = np.array([[90.0, 10.0, nan], [95.0, 10.0, -3.0], [95.0, 20.0, 0.0], [1.0, 99.0, 5.0]], np.float32)
    pair, best = frag_ref.reduce(ani, [0, 3, 3, 4], [0, 1, 3], 20.0)
    assert best["m"].tolist() == [[95000, 20000, 0], [0, 0, 0], [1000, 99000, 5000]]
    assert best["row"].tolist() == [[1, 2, 0], [frag_ref.NONE] * 3, [3, 3, 3]]  # ties to the smaller row, also at 0
    assert pair["total"].tolist() == [[1, 2]] * 3
    assert pair["matched"].tolist() == [[1, 1], [0, 0], [0, 1]] and pair["sum"].tolist() == [[95000, 20000], [0, 0], [0, 99000]]
    pair0, _ = frag_ref.reduce(ani, [0, 3, 3, 4], [0, 1, 3], 0.0)
    assert pair0["matched"].tolist() == [[1, 2]] * 3  # m_th = 0: every fragment matches, a genome without rows too
    assert frag_ref.ani_milli(95000 + 96001, 2) == 95501 and frag_ref.ani_milli(3, 2) == 2 and frag_ref.milli_str(95501) == "95.501"
    assert frag_ref.milli_str(100000) == "100.000" and frag_ref.milli_str(7) == "0.007"
    with pytest.raises(frag_ref.Invalid):
        frag_ref.reduce(ani, [0, 3, 2, 4], [0, 1, 3], 0.0)
    with pytest.raises(frag_ref.Invalid):
        frag_ref.reduce(ani, [0, 3, 3, 4], [0, 1, 2], 0.0)


def test_genomes_of_record_names():
    names = ["a.fna:1-4000", "a.fna:2001-6000", "b.fna", "dir/c.fna:1-10", "dir/c.fna:11-20", "d:x-1", ":1-2"]
    assert frag_ref.genomes(names) == ([0, 2, 3, 5, 6, 7], ["a.fna", "b.fna", "dir/c.fna", "d:x-1", ":1-2"])
    with pytest.raises(frag_ref.Invalid):
        frag_ref.genomes(["a:1-2", "b:1-2", "a:3-4"])
    pair = np.zeros((2, 1), frag_ref.PAIR_DTYPE)
    pair[0, 0], pair[1, 0] = (2 * 96000 + 1, 2, 5), (84999, 1, 5)
    assert frag_ref.tsv(pair, ["r0", "r1"], ["q"], 85.0) == "r0\tq\t96.001\t2\t5\n"  # (96000.5 rounds up; 84.999 is below -a)
    assert frag_ref.tsv(pair, ["r0", "r1"], ["q"], 0.0, min_fragments=2) == "r0\tq\t96.001\t2\t5\n"


# ---- command line ------------------------------------------------------------------------------------------------------------

def run_cli(hg, *args):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")  # (no device: all of this is decided before one is opened)
    return subprocess.run([hg.CLI_PATH, *args], capture_output=True, text=True, env=env)


def test_help_texts_name_the_options_and_the_general_help_does_not(hg):
    general = run_cli(hg, "--help")
    assert general.returncode == 0 and "--fragment" not in general.stdout and "--min_fragments" not in general.stdout
    sk = run_cli(hg, "sketch", "--help")
    assert sk.returncode == 0 and sk.stdout.startswith(general.stdout)
    tail = sk.stdout[len(general.stdout):]
    at = tail.index("\nsketch --fragment W [--fragment_step S]:")
    assert at > tail.index("\nsketch --individual") and "--fragment" not in tail[:at]
    for word in ("multiples of 4", "W / 2", "file:start-end", "1-based", "--fragment 2L --fragment_step L", "--individual", "--alphabet protein",
                 "--translate", "--shards", "first visible GPU"):
        assert word in tail[at:], word
    di = run_cli(hg, "dist", "--help")
    assert di.returncode == 0 and di.stdout.startswith(general.stdout)
    tail = di.stdout[len(general.stdout):]
    at = tail.index("\ndist --fragments [--fragment_ani T] [--min_fragments N] [--fragment_hits FILE]:")
    assert "--fragment" not in tail[:at]
    para = " ".join(tail[at:].split())
    for word in ("--fragment_ani T [90]", "below about 88 are noise", "--min_fragments N [1]", "containment unless it is given", "aligned fraction",
                 "--pairs, --columns, --newick or --shards", "first visible GPU", "by query, then reference", ":start-end"):
        assert word in para, word
    for mode in ("search", "cluster"):
        assert "--fragment" not in run_cli(hg, mode, "--help").stdout


NOT_SKETCH = ": it cuts the sequences sketch reads into windows\n"
CLI_ERRORS = [
    # sketch --fragment / --fragment_step
    (("dist", "--fragment", "1000"), "error: --fragment is not supported by dist" + NOT_SKETCH),
    (("search", "--fragment=1000"), "error: --fragment is not supported by search" + NOT_SKETCH),
    (("cluster", "--fragment_step", "8"), "error: --fragment_step is not supported by cluster" + NOT_SKETCH),
    (("sketch", "--fragment", "1000", "--individual"),
     "error: --fragment is not supported with --individual: the windows are cut from a file's merged sequence, not from its records\n"),
    (("sketch", "--alphabet", "protein", "--fragment", "1000"),
     "error: --fragment is not supported with --alphabet protein: protein input is sketched one file at a time\n"),
    (("sketch", "--fragment", "1000", "--translate"),
     "error: --fragment is not supported with --translate: translated input is sketched one file at a time\n"),
    (("sketch", "--fragment", "1000", "--shards", "2"),
     "error: --shards is not supported with --fragment: the windows are sketched on the first visible GPU\n"),
    (("sketch", "--fragment", "0"), "error: invalid value '0' for '--fragment': a window is a multiple of 4 bases, at least 4\n"),
    (("sketch", "--fragment", "1002"), "error: invalid value '1002' for '--fragment': a window is a multiple of 4 bases, at least 4\n"),
    (("sketch", "--fragment", "1000", "--fragment_step", "0"),
     "error: invalid value '0' for '--fragment_step': a step is a multiple of 4 bases, at least 4\n"),
    (("sketch", "--fragment", "1000", "--fragment_step=502"),
     "error: invalid value '502' for '--fragment_step': a step is a multiple of 4 bases, at least 4\n"),
    (("sketch", "--fragment_step", "1004", "--fragment", "1000"),
     "error: invalid value '1004' for '--fragment_step': a step above the window would leave bases out\n"),
    (("sketch", "--fragment", "20"), "error: invalid value '20' for '--fragment': a window shorter than -k holds no k-mer\n"),
    (("sketch", "--fragment", "32", "-k", "33"), "error: invalid value '32' for '--fragment': a window shorter than -k holds no k-mer\n"),
    (("sketch", "--fragment_step", "500"), "error: --fragment_step needs --fragment: without it sketch makes one sketch per file\n"),
    (("sketch", "--fragment", "x"), "error: invalid value 'x' for '--fragment'\n"),
    (("sketch", "--fragment"), "error: a value is required for '--fragment'\n"),
    # dist --fragments and what belongs to it
    (("sketch", "--fragments"), "error: --fragments is not supported by sketch: it makes dist compare genomes fragment by fragment\n"),
    (("cluster", "--fragments"), "error: --fragments is not supported by cluster: it makes dist compare genomes fragment by fragment\n"),
    (("dist", "--fragments=1"), "error: unexpected argument '--fragments=1'\n"),
    (("search", "--fragment_ani", "95"), "error: --fragment_ani is not supported by search: it belongs to dist --fragments\n"),
    (("dist", "--fragment_ani", "95"), "error: --fragment_ani needs --fragments: without it dist compares whole sketches\n"),
    (("dist", "--min_fragments", "3"), "error: --min_fragments needs --fragments: without it dist compares whole sketches\n"),
    (("dist", "--fragment_hits", "h.tsv"), "error: --fragment_hits needs --fragments: without it dist compares whole sketches\n"),
    (("dist", "--fragments", "--fragment_ani", "101"), "error: invalid value '101' for '--fragment_ani' (an ANI, 0 to 100)\n"),
    (("dist", "--fragments", "--fragment_ani", "ninety"), "error: invalid value 'ninety' for '--fragment_ani' (an ANI, 0 to 100)\n"),
    (("dist", "--fragments", "--min_fragments", "0"), "error: invalid value '0' for '--min_fragments'\n"),
    (("dist", "--fragments", "--fragment_hits", ""), "error: invalid value '' for '--fragment_hits' (a file name)\n"),
    (("dist", "--fragments", "--pairs", "p.tsv"), "error: --pairs is not supported with --fragments: every pair of genomes is compared\n"),
    (("dist", "--columns", "mash", "--fragments"),
     "error: --columns is not supported with --fragments: a line carries the fragment ANI, the matched and the total fragments\n"),
    (("dist", "--fragments", "--newick", "t.nwk", "-r", "a", "-q", "a"),
     "error: --newick is not supported with --fragments: the tree is drawn from whole sketches\n"),
    (("dist", "--fragments", "--shards", "2"), "error: --shards is not supported with --fragments: it runs on the first visible GPU\n"),
    # what is not rejected goes on to the required arguments, as ever
    (("sketch", "--fragment", "4000", "--fragment_step", "2000", "--min_count", "2", "-k", "255"),
     "error: the following required arguments were not provided: --path --out\n"),
    (("sketch", "--fragment=24", "-k", "24"), "error: the following required arguments were not provided: --path --out\n"),
    (("dist", "--fragments", "--fragment_ani=92.5", "--min_fragments", "4", "--fragment_hits=h.tsv", "--ani_metric", "mash"),
     "error: the following required arguments were not provided: --path_r --path_q --out\n"),
]


@pytest.mark.parametrize("args,stderr", CLI_ERRORS)
def test_cli_error_lines(hg, args, stderr, tmp_path):
    r = run_cli(hg, *args)
    assert (r.returncode, r.stdout, r.stderr) == (2, "", stderr)
