"""Neighbour joining (hg_nj*, `hyper-gen dist --newick`), the parts that need no GPU: the C ABI's declarations, exports and
record layout, the command line's surface (what it rejects before a device is opened or a file read, `dist --help`),
hg_nj_newick on literals and malformed join lists, and the CPU models of tests/nj_ref.py -- the sequential rule on Python
integers against its numpy form, on the textbook five-taxon example, on matrices full of ties, on matrices where the clamp
acts and branches come out negative, and on additive matrices, which are recovered exactly."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import nj_ref as nj

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("hg_nj_matrix_dev", "hg_nj_dev", "hg_nj", "hg_nj_newick")

# the textbook example (distances x 1000, in thousandths) and the joins of the rule, lengths in units of 1000 << 15
FIVE = np.array([[0, 5, 9, 9, 8], [5, 0, 10, 10, 9], [9, 10, 0, 8, 7], [9, 10, 8, 0, 3], [8, 9, 7, 3, 0]], np.int64) * 1000
FIVE_JOINS = [(0, 1, 2, 3), (0, 2, 3, 4), (0, 3, 2, 2), (0, 4, 1, 0)]
FIVE_NEWICK = "((('a':0.02000000,'b':0.03000000):0.03000000,'c':0.04000000):0.02000000,'d':0.02000000,'e':0.01000000);"
K = 1000 << 15


@pytest.fixture(scope="module")
def hg():
    import hypergen_amd
    hypergen_amd.lib()
    return hypergen_amd


def run(hg, *args, cwd=None):
    return subprocess.run([hg.CLI_PATH] + list(args), capture_output=True, text=True, timeout=60, cwd=cwd)


# ---- the C ABI ------------------------------------------------------------------------------------------------------
def test_nj_symbols_declared_and_exported(hg):
    hdr_full = open(os.path.join(ROOT, "include", "hypergen.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr_full, flags=re.S)
    nm = subprocess.run(["nm", "-D", "--defined-only", hg.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r"\bT (hg_\w+)", nm))
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NAMES:
        assert re.search(r"\bhg_status %s\(" % name, hdr), name
        assert name in exported, name
        assert name in hg.EXPORTS, name
        assert getattr(hg.lib(), name).argtypes is not None, name
        assert "pub fn %s(" % name in integration, name
    assert re.search(r"#define HG_NJ_FRAC_BITS 15\b", hdr) and re.search(r"#define HG_NJ_MAX_N 65536u\b", hdr)
    assert (hg.NJ_FRAC_BITS, hg.NJ_MAX_N) == (15, 65536) and nj.FRAC_BITS == 15
    assert '"nj_block_rows"' in hdr_full
    for method in ("nj", "nj_dev", "nj_matrix_dev"):
        assert callable(getattr(hg.Context, method)), method
    assert callable(hg.nj_newick)
    # the kernels the header's prose names are in the library
    nmc = subprocess.run(["nm", "-C", hg.LIB_PATH], capture_output=True, text=True).stdout
    named = set(re.findall(r"\bnj_[a-z]+_kernel\b", hdr_full))
    assert {"nj_fill_kernel", "nj_mirror_kernel", "nj_rsum_kernel", "nj_best_kernel", "nj_pick_kernel", "nj_update_kernel"} <= named
    for k in named:
        assert re.search(r"::%s\(" % k, nmc), k


def test_join_record_is_24_bytes_with_the_headers_offsets(hg, tmp_path):
    assert hg.NJ_JOIN_DTYPE.itemsize == 24
    assert [hg.NJ_JOIN_DTYPE.fields[k][1] for k in ("a", "b", "len_a", "len_b")] == [0, 4, 8, 16]
    assert hg.NJ_JOIN_DTYPE == nj.JOIN_DTYPE
    # ... as a C compiler lays the header's struct out
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "hypergen.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu\\n", sizeof(hg_nj_join), offsetof(hg_nj_join, a), offsetof(hg_nj_join, b),\n'
                   '                        offsetof(hg_nj_join, len_a), offsetof(hg_nj_join, len_b)); return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert subprocess.run([str(exe)], capture_output=True, text=True).stdout == "24 0 4 8 16\n"


# ---- the command line -----------------------------------------------------------------------------------------------
def test_the_option_table_has_the_newick_row_and_stays_within_the_width_of_given():
    src = open(os.path.join(ROOT, "hyper-gen_amd", "csrc", "hg_cli.cpp")).read()
    table = src[src.index("const Option options[] = {"):src.index("const size_t N_OPTIONS")]
    rows = re.findall(r"^    \{\"([a-z_]+)\", ", table, flags=re.M)
    width, = map(int, re.findall(r"std::bitset<(\d+)> given;", src))  # Cli::given, a bit per row
    assert width == 64 and "newick" in rows and len(rows) == len(set(rows)) == 40 <= width


NOT_DIST = "error: --newick is not supported by %s: it draws the tree of dist's comparison\n"
ONE_FILE = "error: --newick needs one sketch file: -r and -q must name the same file\n"
FAULTS = [
    (("sketch", "--newick", "t.nwk"), NOT_DIST % "sketch"),
    (("search", "--newick", "t.nwk"), NOT_DIST % "search"),
    (("cluster", "--newick=t.nwk"), NOT_DIST % "cluster"),
    (("dist", "--newick", ""), "error: invalid value '' for '--newick' (a file name)\n"),
    (("dist", "--newick="), "error: invalid value '' for '--newick' (a file name)\n"),
    (("dist", "--newick", "t.nwk", "--ani_metric", "containment"),
     "error: --ani_metric containment is not supported with --newick: it is directional (mash | max_containment)\n"),
    (("dist", "--newick", "t.nwk", "--pairs", "p.tsv"),
     "error: --pairs is not supported with --newick: the tree needs every pair, not the listed ones\n"),
    (("dist", "--newick", "t.nwk", "--shards", "2"),
     "error: --newick is not supported with --shards: dist with --columns or --pairs runs on the first visible GPU\n"),
]


@pytest.mark.parametrize("args,err", FAULTS, ids=[" ".join(a) for a, _ in FAULTS])
def test_rejected_before_any_device_or_file(hg, tmp_path, args, err):
    missing = str(tmp_path / "missing.sketch")
    paths = ("-p", missing) if args[0] in ("cluster", "sketch") else ("-r", missing, "-q", missing)
    r = run(hg, *args, *paths, "-o", "out.tsv", cwd=str(tmp_path))
    assert (r.returncode, r.stderr, r.stdout) == (2, err, "")
    assert os.listdir(str(tmp_path)) == []


def test_two_different_files_are_refused(hg, tmp_path):
    for extra in ((), ("--ani_metric", "containment"), ("--pairs", "p.tsv")):  # (reported before the other two)
        r = run(hg, "dist", "--newick", "t.nwk", "-r", "a.sketch", "-q", "b.sketch", "-o", "out.tsv", *extra, cwd=str(tmp_path))
        assert (r.returncode, r.stderr, r.stdout) == (2, ONE_FILE, "")
    r = run(hg, "dist", "--newick", "t.nwk", "-r", "a.sketch", "-o", "out.tsv", cwd=str(tmp_path))
    assert (r.returncode, r.stderr, r.stdout) == (2, ONE_FILE, "")
    # accepted up to the required arguments
    r = run(hg, "dist", "--newick", "t.nwk", "--ani_metric", "max_containment", "--columns", "mash", cwd=str(tmp_path))
    assert (r.returncode, r.stderr) == (2, "error: the following required arguments were not provided: --path_r --path_q --out\n")
    assert os.listdir(str(tmp_path)) == []


@pytest.mark.parametrize("flag", ["--help", "-h"])
def test_dist_help_is_the_general_help_and_one_paragraph(hg, tmp_path, flag):
    general = run(hg, "--help", cwd=str(tmp_path))
    r = run(hg, "dist", flag, cwd=str(tmp_path))
    assert (r.returncode, r.stderr) == (0, "")
    assert r.stdout.startswith(general.stdout) and len(r.stdout) > len(general.stdout)
    paragraphs = [p for p in r.stdout[len(general.stdout):].split("\n\n") if p.strip()]
    assert len(paragraphs) == 1 and paragraphs[0].strip().startswith("dist --newick <file>:")
    para = " ".join(paragraphs[0].split())
    for phrase in ("neighbour joining", "(c - 2) d(i, j) - r(i) - r(j)", "100 - ANI", "single quotes", "doubled", "unrooted", "three children",
                   "negative", "4 bytes per pair", "65536", "-o is what it is without --newick"):
        assert phrase in para, phrase
    assert "--newick" not in general.stdout
    assert run(hg, "cluster", "--help", cwd=str(tmp_path)).stdout.count("--newick") == 0
    assert os.listdir(str(tmp_path)) == []


# ---- hg_nj_newick ---------------------------------------------------------------------------------------------------
def scaled(joins, k=K):
    return nj.as_records([(a, b, la * k, lb * k) for a, b, la, lb in joins])


def test_newick_literals(hg):
    assert hg.nj_newick(scaled([]), ["only"]) == "'only';"
    assert hg.nj_newick(scaled([(0, 1, 7, 0)]), ["a", "b"]) == "('a':0.07000000,'b':0.00000000);"
    # three: the top level lists the two children of the first join and the other side of the last, by name
    assert hg.nj_newick(scaled([(0, 1, 1, 2), (0, 2, 3, 0)]), ["x", "y", "z"]) == "('x':0.01000000,'y':0.02000000,'z':0.03000000);"
    assert hg.nj_newick(scaled([(1, 2, 1, 2), (0, 1, 3, 0)]), ["x", "y", "z"]) == "('x':0.03000000,'y':0.01000000,'z':0.02000000);"
    assert hg.nj_newick(scaled([(0, 2, 1, 2), (0, 1, 3, 0)]), ["x", "y", "z"]) == "('x':0.01000000,'y':0.03000000,'z':0.02000000);"
    assert hg.nj_newick(scaled(FIVE_JOINS), list("abcde")) == FIVE_NEWICK
    assert hg.nj_newick(scaled(FIVE_JOINS), [b"a", b"b", b"c", b"d", b"e"]) == FIVE_NEWICK  # (bytes as the .sketch file carries them)
    assert nj.newick_model(nj.as_tuples(scaled(FIVE_JOINS)), "abcde") == FIVE_NEWICK


def test_newick_quotes_every_label(hg):
    names = ["it's (a: b)", "dir/g 1.fna", "''", ""]
    joins = scaled([(0, 1, 1, 1), (2, 3, 1, 1), (0, 2, 1, 0)])
    # (the second-to-last join is (2, 3): its two children and, first by name, the other side of the last join)
    want = "(('it''s (a: b)':0.01000000,'dir/g 1.fna':0.01000000):0.01000000,'''''':0.01000000,'':0.01000000);"
    assert hg.nj_newick(joins, names) == want == nj.newick_model(nj.as_tuples(joins), names)


def test_newick_lengths_by_integers(hg):
    def one(length):
        text = hg.nj_newick(nj.as_records([(0, 1, length, 0)]), ["a", "b"])
        assert text == "('a':%s,'b':0.00000000);" % nj.newick_length(length)
        return text[5:text.index(",")]

    assert one(0) == "0.00000000" and one(K) == "0.01000000" and one(-K) == "-0.01000000"
    assert one(100_000 << 15) == "1.00000000" and one(-(100_000 << 15)) == "-1.00000000"
    # one unit is 2^-15 thousandths: t = (|len| * 1000 + 16384) >> 15 rounds to the nearest 1e-8, halves up
    assert one(16) == "0.00000000" and one(17) == "0.00000001" and one(-16) == "0.00000000" and one(-17) == "-0.00000001"
    assert one(1 << 15) == "0.00001000" and one((1 << 15) + 1) == "0.00001000" and one(12345 << 15) == "0.12345000"
    assert one((3 << 15) // 2) == "0.00001500"
    assert one((1 << 62) + 5) == nj.newick_length((1 << 62) + 5) and one(-(1 << 63)) == nj.newick_length(-(1 << 63))  # no overflow


INVALID = [
    ("a equals b", 3, [(0, 0, 1, 1), (0, 1, 1, 0)]),
    ("a above b", 3, [(1, 0, 1, 1), (0, 2, 1, 0)]),
    ("a name beyond n", 3, [(0, 3, 1, 1), (0, 1, 1, 0)]),
    ("a name far beyond n", 3, [(0, 0xFFFFFFFF, 1, 1), (0, 1, 1, 0)]),
    ("a dead name as b", 3, [(0, 1, 1, 1), (0, 1, 1, 0)]),
    ("a dead name as a", 4, [(0, 1, 1, 1), (1, 2, 1, 1), (0, 3, 1, 0)]),
    ("two names", 2, [(1, 1, 1, 0)]),
]


@pytest.mark.parametrize("what,n,joins", INVALID, ids=[x[0] for x in INVALID])
def test_newick_refuses_malformed_join_lists(hg, what, n, joins):
    with pytest.raises(hg.HgError) as e:
        hg.nj_newick(nj.as_records(joins), ["n%d" % i for i in range(n)])
    assert e.value.status == hg.ERR_INVALID


def test_newick_null_arguments_and_no_items(hg):
    lib = hg.lib()
    p, ln = C.c_void_p(), C.c_size_t(7)
    names = (C.c_char_p * 2)(b"a", b"b")
    j = nj.as_records([(0, 1, 1, 0)])
    jp = C.c_void_p(j.ctypes.data)
    assert lib.hg_nj_newick(jp, 2, names, None, C.byref(ln)) == hg.ERR_INVALID
    assert lib.hg_nj_newick(None, 2, names, C.byref(p), C.byref(ln)) == hg.ERR_INVALID and not p.value and ln.value == 0
    assert lib.hg_nj_newick(jp, 2, None, C.byref(p), C.byref(ln)) == hg.ERR_INVALID
    assert lib.hg_nj_newick(jp, 0, names, C.byref(p), C.byref(ln)) == hg.ERR_INVALID
    assert lib.hg_nj_newick(jp, 2, (C.c_char_p * 2)(b"a", None), C.byref(p), C.byref(ln)) == hg.ERR_INVALID
    assert lib.hg_nj_newick(jp, 2, names, C.byref(p), None) == hg.OK  # (len may be NULL)
    assert C.string_at(p) == b"('a':0.00000000,'b':0.00000000);"
    lib.hg_free(p)
    with pytest.raises(hg.HgError):
        hg.nj_newick(nj.as_records([]), [])
    with pytest.raises(hg.HgError):
        hg.nj_newick(nj.as_records([(0, 1, 1, 0)]), ["a", "b", "c"])


def test_newick_of_a_caterpillar_of_many_leaves(hg):
    n = 30_000  # (as deep as a tree gets: nothing recurses)
    joins = nj.as_records([(0, t + 1, 1 << 15, 2 << 15) for t in range(n - 1)])
    text = hg.nj_newick(joins, [str(i) for i in range(n)])
    assert text.startswith("(" * (n - 2) + "'0':0.00001000,'1':0.00002000)") and text.endswith(",'%d':0.00003000);" % (n - 1))
    assert text.count("(") == text.count(")") == n - 2


# ---- the models -----------------------------------------------------------------------------------------------------
def test_model_five_taxa(hg):
    d = FIVE << 15
    want = [(a, b, la * K, lb * K) for a, b, la, lb in FIVE_JOINS]
    assert nj.nj_model(d) == want and nj.nj_model_np(d) == want
    # the same through the float matrix, of which only the upper triangle counts
    a = nj.ani_of_milli(FIVE)
    a[np.tril_indices(5)] = np.nan
    assert np.array_equal(nj.dist_matrix(a), d)
    # both ties of the example.  Second round, u = (a, b): Q(u, c) = Q(d, e) = -28 000, the lower name wins ...
    d2 = np.array([[0, 7, 7, 6], [7, 0, 8, 7], [7, 8, 0, 3], [6, 7, 3, 0]], np.int64) * K
    r = d2.sum(axis=1)
    q = 2 * d2 - r[:, None] - r[None, :]
    assert q[0, 1] == q[2, 3] == q[np.triu_indices(4, 1)].min() == -28 * K and (q[np.triu_indices(4, 1)] == -28 * K).sum() == 2
    assert nj.nj_model(d2)[0] == (0, 1, 3 * K, 4 * K)
    # ... third round, v = (u, c): all three pairs at -10 000
    d3 = np.array([[0, 4, 3], [4, 0, 3], [3, 3, 0]], np.int64) * K
    r = d3.sum(axis=1)
    q = d3 - r[:, None] - r[None, :]
    assert (q[np.triu_indices(3, 1)] == -10 * K).all()
    assert nj.nj_model(d3) == [(0, 1, 2 * K, 2 * K), (0, 2, 1 * K, 0)]


def test_model_smallest_inputs():
    assert nj.nj_model(np.zeros((0, 0), np.int64)) == [] == nj.nj_model_np(np.zeros((0, 0), np.int64))
    assert nj.nj_model(np.zeros((1, 1), np.int64)) == [] == nj.nj_model_np(np.zeros((1, 1), np.int64))
    d = np.array([[0, 77], [77, 0]], np.int64)
    assert nj.nj_model(d) == [(0, 1, 77, 0)] == nj.nj_model_np(d)
    d = np.array([[0, 3, 4], [3, 0, 6], [4, 6, 0]], np.int64)  # c = 3: Q = d - r - r; len_a = floor((3 + 7 - 9) / 2) = 0
    assert nj.nj_model(d) == [(0, 1, 0, 3), (0, 2, 3, 0)] == nj.nj_model_np(d)  # (all three Q equal: the lowest names)
    d = np.array([[0, 3, 9], [3, 0, 4], [9, 4, 0]], np.int64)  # a negative numerator: floor((3 + 12 - 7) / 2), then (1, 2)...
    assert nj.nj_model(d) == nj.nj_model_np(d)


def random_ani(rng, n, kind):
    if kind == "ties":  # three distinct values: ties decide nearly every join
        a = rng.choice(np.array([95.0, 97.0, 99.0], np.float32), (n, n))
    elif kind == "wide":  # over 0 .. 100 000: far from a tree, the clamp acts and branches come out negative
        a = (rng.integers(0, 100_001, (n, n)) / 1000.0).astype(np.float32)
    else:  # clustered: groups at 96 .. 99.9, 80 .. 90 between them
        a = rng.uniform(80.0, 90.0, (n, n))
        g = rng.integers(0, max(2, n // 6), n)
        within = g[:, None] == g[None, :]
        a[within] = rng.uniform(96.0, 99.9, int(within.sum()))
        a = a.astype(np.float32)
    a = np.triu(a, 1)
    return a + a.T


def test_both_forms_of_the_model_are_identical():
    rng = np.random.default_rng(11)
    negative = clamped = tied = 0
    for k in range(240):
        n = int(rng.integers(2, 26))
        kind = ("ties", "wide", "clustered")[k % 3]
        a = random_ani(rng, n, kind)
        d = nj.dist_matrix(a)
        stats = {"clamped": 0}
        seq = nj.nj_model(d, stats if kind == "wide" else None)
        clamped += stats["clamped"]
        assert seq == nj.nj_model_np(d), (k, n, kind)
        assert len(seq) == n - 1 and all(x < y < n for x, y, _, _ in seq) and seq[-1][3] == 0
        assert sorted(y for _, y, _, _ in seq) == sorted(set(range(n)) - {seq[-1][0]})  # every name but one dies, once
        negative += sum(la < 0 or lb < 0 for _, _, la, lb in seq)
        if kind == "ties":
            r = d.sum(axis=1)
            q = (n - 2) * d - r[:, None] - r[None, :]
            up = q[np.triu_indices(n, 1)]
            tied += int((up == up.min()).sum() > 1)
        # the lower triangle and the diagonal of the float matrix are not read
        b = a.copy()
        b[np.tril_indices(n)] = rng.uniform(-1e9, 1e9)
        assert np.array_equal(nj.dist_matrix(b), d)
    print("joins with a negative branch: %d, updates the clamp acted on: %d, first rounds with a tie: %d" % (negative, clamped, tied))
    assert negative > 20 and clamped > 5 and tied > 20


def test_additive_matrices_are_recovered_exactly():
    rng = np.random.default_rng(2)
    for n in range(2, 71):
        t = nj.additive_matrix(rng, n)
        d = nj.dist_matrix(nj.ani_of_milli(t))
        assert np.array_equal(d, t << 15)
        joins = nj.nj_model_np(d)
        if n <= 24:
            assert joins == nj.nj_model(d), n
        assert np.array_equal(nj.path_lengths(joins, n), d), n  # topology and every branch
        assert all(la >= 0 and lb >= 0 and la % (1 << 15) == 0 and lb % (1 << 15) == 0 for _, _, la, lb in joins), n


def test_values_outside_0_100_count_as_dist_prints_them():
    a = np.array([[0, np.nan, -3.0, 250.0], [0, 0, 99.9996, 99.9994], [0, 0, 0, np.inf], [0, 0, 0, 0]], np.float32)
    m = nj.milli_matrix(a)
    assert m[0, 1] == 0 and m[0, 2] == 0 and m[0, 3] == 100_000 and m[1, 2] == 100_000 and m[1, 3] == 99_999 and m[2, 3] == 100_000
    d = nj.dist_matrix(a)
    assert d[0, 1] == d[1, 0] == 100_000 << 15 and d[1, 3] == 1 << 15 and d[0, 3] == 0
