"""Average linkage (hg_cluster_average*, `hyper-gen cluster --hclust average`), the parts that need no GPU: the C ABI's
declarations and exports, the command line's surface (cluster --help, what it rejects before a device is opened or a file
read), the CPU models of tests/cluster_average_ref.py on hand-written cases and against each other, and the exact
comparison of hg_average_cmp.h in a stand-alone host program against Python integers -- with operands whose cross
products differ only above bit 64, which no shape of the device tests reaches."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import cluster_average_ref as av

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("hg_cluster_average_matrix_dev", "hg_cluster_average_dev", "hg_cluster_average", "hg_ctx_cluster_average_rounds")


@pytest.fixture(scope="module")
def hg():
    import hypergen_amd
    hypergen_amd.lib()
    return hypergen_amd


def run(hg, *args, cwd=None):
    return subprocess.run([hg.CLI_PATH] + list(args), capture_output=True, text=True, timeout=60, cwd=cwd)


def test_average_symbols_declared_and_exported(hg):
    hdr_full = open(os.path.join(ROOT, "include", "hypergen.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr_full, flags=re.S)
    nm = subprocess.run(["nm", "-D", "--defined-only", hg.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r"\bT (hg_\w+)", nm))
    for name in NAMES:
        assert re.search(r"\b(hg_status|uint64_t) %s\(" % name, hdr), name
        assert name in exported, name
        assert name in hg.EXPORTS, name
        assert getattr(hg.lib(), name).argtypes is not None, name
    assert re.search(r"#define HG_CLUSTER_AVERAGE_MAX_N 65536u\b", hdr)
    assert hg.CLUSTER_AVERAGE_MAX_N == 65536
    assert '"average_rounds"' in hdr_full and '"average_block_rows"' in hdr_full
    # six outputs behind the threshold: rep, cluster, into, level, size, n_clusters
    assert len(hg.lib().hg_cluster_average_matrix_dev.argtypes) == 10
    assert len(hg.lib().hg_cluster_average_dev.argtypes) == len(hg.lib().hg_cluster_average.argtypes) == 13
    for method in ("cluster_average", "cluster_average_dev", "cluster_average_matrix_dev", "cluster_average_rounds"):
        assert callable(getattr(hg.Context, method)), method
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NAMES:
        assert "pub fn %s(" % name in integration, name


def test_cluster_help_names_hclust_and_keeps_the_general_help(hg, tmp_path):
    general = run(hg, "--help", cwd=str(tmp_path))
    r = run(hg, "cluster", "--help", cwd=str(tmp_path))
    assert (r.returncode, r.stderr) == (0, "")
    assert r.stdout.startswith(general.stdout) and len(r.stdout) > len(general.stdout)
    tail = r.stdout[len(general.stdout):]
    assert "--hclust average" in tail and "--tree" in tail
    assert "--hclust" not in general.stdout
    assert os.listdir(str(tmp_path)) == []


FAULTS = [
    (("cluster", "--hclust", "x"), "error: invalid value 'x' for '--hclust' (average)\n"),
    (("cluster", "--hclust", "single"), "error: invalid value 'single' for '--hclust' (average)\n"),
    (("cluster", "--hclust", "average", "--linkage", "single"),
     "error: --hclust does not go with --linkage: average linkage is a scheme of its own, not one of --linkage's\n"),
    (("cluster", "--linkage", "greedy", "--hclust=average"),
     "error: --hclust does not go with --linkage: average linkage is a scheme of its own, not one of --linkage's\n"),
    (("cluster", "--hclust", "average", "--levels", "97,99"),
     "error: --levels is not supported with --hclust: it cuts the single-linkage tree, not the dendrogram of average linkage\n"),
    (("cluster", "--hclust", "average", "--tree", "t.tsv", "--levels", "97"),
     "error: --levels is not supported with --hclust: it cuts the single-linkage tree, not the dendrogram of average linkage\n"),
    # the present messages of the options that do not go with cluster, or with anything but greedy
    (("cluster", "--hclust", "average", "--order", "size"),
     "error: --order needs cluster --linkage greedy: single-linkage components do not depend on the order of the sketches\n"),
    (("cluster", "--hclust", "average", "--shards", "2"), "error: --shards is not supported by cluster: it runs on the first visible GPU\n"),
    (("cluster", "--hclust", "average", "--ani_metric", "containment"),
     "error: --ani_metric containment is not supported by cluster: it is directional (mash | max_containment)\n"),
    # the other subcommands refuse the option with the table's sentence
    (("sketch", "--hclust", "average"), "error: --hclust is not supported by sketch: it chooses the hierarchical clustering of cluster\n"),
    (("dist", "--hclust", "average"), "error: --hclust is not supported by dist: it chooses the hierarchical clustering of cluster\n"),
    (("search", "--hclust", "average"), "error: --hclust is not supported by search: it chooses the hierarchical clustering of cluster\n"),
]


@pytest.mark.parametrize("args,err", FAULTS, ids=[" ".join(a) for a, _ in FAULTS])
def test_rejected_before_any_device_or_file(hg, tmp_path, args, err):
    # the input does not exist and no device is needed: the option is refused first, and nothing is created
    missing = str(tmp_path / "missing.sketch")
    paths = ("-p", missing) if args[0] in ("cluster", "sketch") else ("-r", missing, "-q", missing)
    r = run(hg, *args, *paths, "-o", "out.tsv", cwd=str(tmp_path))
    assert (r.returncode, r.stderr, r.stdout) == (2, err, "")
    assert os.listdir(str(tmp_path)) == []


def test_hclust_with_tree_is_accepted_up_to_the_required_arguments(hg, tmp_path):
    r = run(hg, "cluster", "--hclust", "average", "--tree", "t.tsv", cwd=str(tmp_path))
    assert (r.returncode, r.stderr) == (2, "error: the following required arguments were not provided: --path --out\n")
    assert os.listdir(str(tmp_path)) == []


# ---- milli ---------------------------------------------------------------------------------------------------------
def test_milli_is_what_dist_prints_on_exact_ties():
    for ani, want in ((12.3125, 12312), (0.1875, 188), (96.0625, 96062), (99.9375, 99938)):
        assert np.float32(ani) == ani  # exactly representable: ani * 1000 ends in .5, a tie
        assert av.milli(ani) == want
        assert "%.3f" % ani == "%d.%03d" % (want // 1000, want % 1000)
    assert av.milli(np.nan) == 0 and av.milli(-1.0) == 0 and av.milli(101.0) == 100_000
    assert av.milli(-0.0) == 0 and av.milli(np.inf) == 100_000 and av.milli(-np.inf) == 0
    assert av.milli(100.0) == 100_000 and av.milli(95.0) == 95_000
    rng = np.random.default_rng(1)
    x = rng.uniform(0, 100, 2000).astype(np.float32)
    assert av.milli_matrix(x).tolist() == [av.milli(v) for v in x] == [int(round(float("%.3f" % v) * 1000)) for v in x]
    assert av.th_milli(np.nan) is None and av.th_milli(100.001) is None and av.th_milli(100.0) == 100_000
    assert av.th_milli(-3.0) == 0 and av.th_milli(0.0) == 0


# ---- the models on hand-written cases ------------------------------------------------------------------------------
def matrix(n, pairs, fill=0.0):
    a = np.full((n, n), fill, np.float32)
    for (i, j), v in pairs.items():
        a[i, j] = a[j, i] = v
    return a


def both(a, th):
    seq = av.average_model(a, th)
    rnd = av.average_model_rounds(a, th)
    for x, y in zip(seq[:5], rnd[:5]):
        assert x.dtype == y.dtype and np.array_equal(x.view(np.uint32), y.view(np.uint32))
    assert seq[5] == rnd[5]
    return seq


def test_model_two_items_at_the_threshold_and_below():
    th = 95.0
    rep, cl, into, level, size, nc = both(matrix(2, {(0, 1): 95.0}), th)
    assert (rep.tolist(), cl.tolist(), into.tolist(), size.tolist(), nc) == ([0, 0], [0, 0], [0, 0], [2, 2], 1)
    assert level.tolist() == [0.0, float(np.float32(95.0))]
    # 94.9995 is the largest float32 that still prints 95.000 -- or not: what counts is milli, not the float comparison
    below = np.nextafter(np.float32(94.9995), np.float32(0))
    assert av.milli(below) == 94_999
    rep, cl, into, level, size, nc = both(matrix(2, {(0, 1): below}), th)
    assert (rep.tolist(), cl.tolist(), into.tolist(), level.tolist(), size.tolist(), nc) == ([0, 1], [0, 1], [0, 1], [0.0, 0.0], [1, 1], 2)
    just = np.float32(94.9996)
    assert just < np.float32(95.0) and av.milli(just) == 95_000
    assert both(matrix(2, {(0, 1): just}), th)[5] == 1  # (below 95 as a float, 95.000 as dist prints it)
    assert both(matrix(2, {(0, 1): 99.0}), np.nan)[5] == 2 and both(matrix(2, {(0, 1): 100.0}), 100.5)[5] == 2
    assert both(matrix(2, {(0, 1): 100.0}), 100.0)[5] == 1 and both(matrix(2, {(0, 1): 0.0}), 0.0)[5] == 1
    assert both(matrix(2, {(0, 1): np.nan}), -1.0)[5] == 1


def test_model_chain_of_three_is_two_clusters_where_single_linkage_gives_one():
    a = matrix(3, {(0, 1): 96.0, (1, 2): 96.0, (0, 2): 0.0})
    rep, cl, into, level, size, nc = both(a, 95.0)
    # {0, 1} first (the smaller lower name of two equal pairs); then S({0, 1}, 2) = 96 000 over 2 pairs = 48: below 95
    assert (rep.tolist(), cl.tolist(), into.tolist(), size.tolist(), nc) == ([0, 0, 2], [0, 0, 1], [0, 0, 2], [2, 2, 1], 2)
    assert level.tolist() == [0.0, 96.0, 0.0]
    # single linkage at 95: one component
    comp = list(range(3))
    for i in range(3):
        for j in range(i + 1, 3):
            if a[i, j] >= 95.0:
                comp = [min(comp[i], comp[j]) if c in (comp[i], comp[j]) else c for c in comp]
    assert len(set(comp)) == 1
    # at 48 the third joins, at the average of the two pairs
    rep, cl, into, level, size, nc = both(a, 48.0)
    assert (into.tolist(), size.tolist(), nc) == ([0, 0, 0], [3, 2, 3], 1) and level.tolist() == [0.0, 96.0, 48.0]
    assert both(a, 48.001)[5] == 2


def test_model_index_tie():
    # all six pairs equal: {0, 1} merges first, then {0 u 1, 2} (lower name 0 beats {2, 3}), then 3
    rep, cl, into, level, size, nc = both(matrix(4, {}, fill=97.0), 95.0)
    assert (into.tolist(), size.tolist(), nc) == ([0, 0, 0, 0], [4, 2, 3, 4], 1)
    # {1, 2} and {0, 3} equal and best: {0, 3} has the smaller lower name; both merge either way, then with each other
    a = matrix(4, {(1, 2): 99.0, (0, 3): 99.0}, fill=96.0)
    rep, cl, into, level, size, nc = both(a, 95.0)
    assert (into.tolist(), size.tolist(), nc) == ([0, 0, 1, 0], [4, 4, 2, 2], 1)
    assert level.tolist() == [0.0, 96.0, 99.0, 99.0]
    # the higher name decides between {0, 1} and {0, 2}
    a = matrix(3, {(0, 1): 98.0, (0, 2): 98.0, (1, 2): 90.0})
    assert both(a, 97.0)[2].tolist() == [0, 0, 2]


def test_model_two_pairs_of_one_round_get_their_cross_sum():
    a = matrix(4, {(0, 1): 99.0, (2, 3): 98.0, (0, 2): 90.0, (0, 3): 91.0, (1, 2): 92.0, (1, 3): 93.0})
    rep, cl, into, level, size, nc, rounds = av.average_model_rounds(a, 91.5, with_rounds=True)
    assert (into.tolist(), size.tolist(), nc, rounds) == ([0, 0, 0, 2], [4, 2, 4, 2], 1, 3)
    assert level[2] == np.float32((90000 + 91000 + 92000 + 93000) / 4 / 1000.0)
    assert av.average_model_rounds(a, 91.501)[5] == 2
    both(a, 91.5)


def random_matrix(rng, n, kind):
    if kind == "ties":
        a = rng.integers(0, 4, (n, n)).astype(np.float32)  # milli in {0, 1000, 2000, 3000}: ties everywhere
    elif kind == "coarse":
        a = (rng.integers(0, 4, (n, n)) * 25.0).astype(np.float32)
    else:
        a = rng.uniform(70.0, 100.0, (n, n)).astype(np.float32)
    a = np.triu(a, 1)
    return a + a.T


def test_sequential_model_equals_round_model():
    rng = np.random.default_rng(7)
    merged = 0
    for k in range(360):
        n = int(rng.integers(2, 14))
        kind = ("ties", "coarse", "uniform")[k % 3]
        a = random_matrix(rng, n, kind)
        th = {"ties": float(rng.integers(0, 4)), "coarse": float(rng.choice([0.0, 25.0, 40.0, 75.0])),
              "uniform": float(rng.uniform(70.0, 95.0))}[kind]
        got = both(a, th)
        merged += n - got[5]
        # the lower triangle and the diagonal are not read
        b = a.copy()
        b[np.tril_indices(n)] = np.nan
        assert all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(av.average_model(b, th)[:5], got[:5]))
    assert merged > 500
    for n, th in ((40, 80.0), (60, 0.0)):
        a = random_matrix(rng, n, "uniform")
        assert both(a, th)[5] == (1 if th == 0.0 else both(a, th)[5])


def test_merge_order_puts_children_before_parents():
    rng = np.random.default_rng(3)
    for kind in ("ties", "uniform", "coarse"):
        a = random_matrix(rng, 60, kind)
        rep, cl, into, level, size, nc = av.average_model_rounds(a, 0.0)
        assert nc == 1
        order = av.merge_order(into, level, size)
        assert len(order) == 59
        built = {i: 1 for i in range(60)}  # name -> current size, replaying the merges in the listed order
        gone = set()
        for b in order:
            assert b not in gone and int(into[b]) not in gone and into[b] < b
            built[int(into[b])] += built[b]
            assert built[int(into[b])] == size[b]  # every merge below this one has been listed: children come first
            gone.add(b)
        # monotone: the level of a merge is not above the levels of the merges inside its two clusters
        for b in order:
            kids = [x for x in order if into[x] == b] + [x for x in order if into[x] == into[b] and size[x] < size[b]]
            assert all(level[x] >= level[b] for x in kids)


# ---- the exact comparison, on the CPU ------------------------------------------------------------------------------
@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_exact_comparison_above_64_bits_against_python_integers(tmp_path):
    exe = tmp_path / "average_cmp_driver"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "native", "average_cmp_driver.cpp"), "-o", str(exe)])
    rng = np.random.default_rng(11)
    cases = []
    # products that differ only above bit 64: sa * db = x * 2^64 + low, sb * da = y * 2^64 + low with the same low 64 bits
    for _ in range(200):
        da = int(rng.integers(1, 1 << 30)) | 1
        db = da + 2 * int(rng.integers(1, 1 << 20))
        sa = int(rng.integers(1 << 46, 1 << 47))
        # choose sb so that sb * da - sa * db is a multiple of 2^64: da is odd, so it has an inverse mod 2^64
        inv = pow(da, -1, 1 << 64)
        sb = (sa * db * inv) % (1 << 64)
        cases.append((sa, da, sb, db))
    # the sizes of the rule itself near the limit: S up to 100 000 c c', denominators up to 2^30
    for _ in range(200):
        ca, cb, cc, cd = (int(x) for x in rng.integers(1, 1 << 15, 4))
        sa, sb = int(rng.integers(0, 100_001)) * ca * cb, int(rng.integers(0, 100_001)) * cc * cd
        cases.append((sa, ca * cb, sb, cc * cd))
        cases.append((sa, ca * cb, sa * cc * cd, ca * cb * cc * cd))  # equal averages
    cases += [(0, 1, 0, 1), ((1 << 64) - 1, 1, (1 << 64) - 1, 1), ((1 << 64) - 1, (1 << 64) - 1, (1 << 64) - 2, (1 << 64) - 1),
              ((1 << 64) - 1, (1 << 64) - 2, (1 << 64) - 1, (1 << 64) - 1), (1 << 63, 3, (1 << 63) + 1, 3)]
    cases = [c for c in cases if all(0 <= v < (1 << 64) for v in c) and c[1] > 0 and c[3] > 0]
    high_only = sum(1 for sa, da, sb, db in cases if (sa * db) % (1 << 64) == (sb * da) % (1 << 64) and sa * db != sb * da)
    assert high_only >= 150
    floats = np.concatenate([np.array([12.3125, 0.1875, 96.0625, 99.9375, np.nan, -1.0, 101.0, -0.0, np.inf, 100.0], np.float32),
                             rng.uniform(0, 100, 500).astype(np.float32)])
    text = "".join("c %d %d %d %d\n" % c for c in cases) + "".join("m %08x\n" % b for b in floats.view(np.uint32))
    out = subprocess.run([str(exe)], input=text, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "average cmp driver ok" in out.stderr, out.stdout[-2000:] + out.stderr
    answers = out.stdout.split()
    assert len(answers) == len(cases) + floats.size
    for (sa, da, sb, db), got in zip(cases, answers):
        l, r = sa * db, sb * da
        assert int(got) == (l > r) - (l < r), (sa, da, sb, db)
    assert [int(x) for x in answers[len(cases):]] == [av.milli(f) for f in floats]
