"""Complete linkage (hg_cluster_complete*, `hyper-gen cluster --agglomerate complete`), the parts that need no GPU: the C
ABI's declarations and exports, the command line's surface (cluster --help, what it rejects before a device is opened or a
file read), and the CPU models of tests/cluster_complete_ref.py on hand-written cases, against each other -- the
sequential rule, the round form with and without the retire and rescan rules -- and, where scipy is installed, against
scipy's linkage(method="complete")."""
import os
import re
import subprocess

import numpy as np
import pytest

import cluster_complete_ref as cp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("hg_cluster_complete_matrix_dev", "hg_cluster_complete_dev", "hg_cluster_complete", "hg_ctx_cluster_complete_rounds")


@pytest.fixture(scope="module")
def hg():
    import hypergen_amd
    hypergen_amd.lib()
    return hypergen_amd


def run(hg, *args, cwd=None):
    return subprocess.run([hg.CLI_PATH] + list(args), capture_output=True, text=True, timeout=60, cwd=cwd)


def test_complete_symbols_declared_and_exported(hg):
    hdr_full = open(os.path.join(ROOT, "include", "hypergen.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr_full, flags=re.S)
    nm = subprocess.run(["nm", "-D", "--defined-only", hg.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r"\bT (hg_\w+)", nm))
    for name in NAMES:
        assert re.search(r"\b(hg_status|uint64_t) %s\(" % name, hdr), name
        assert name in exported, name
        assert name in hg.EXPORTS, name
        assert getattr(hg.lib(), name).argtypes is not None, name
    assert re.search(r"#define HG_CLUSTER_COMPLETE_MAX_N 65536u\b", hdr)
    assert hg.CLUSTER_COMPLETE_MAX_N == 65536
    for key in ('"complete_rounds"', '"complete_block_rows"', '"complete_rescan"'):
        assert key in hdr_full, key
    # the two lists of entry points that depend on the ANI metric, and the one of those that take the matrix
    assert hdr_full.count("hg_cluster_complete{,_dev}") == 2
    assert re.search(r"hg_cluster_complete_matrix_dev and hg_cluster_stats_matrix_dev \(they take the matrix\)", hdr_full)
    # the prototypes and the argument order of hg_cluster_average*
    lib = hg.lib()
    for kind in ("_matrix_dev", "_dev", ""):
        a, c = getattr(lib, "hg_cluster_average" + kind), getattr(lib, "hg_cluster_complete" + kind)
        assert (c.restype, list(c.argtypes)) == (a.restype, list(a.argtypes)), kind
        decl = {k: re.search(r"hg_status hg_cluster_%s%s\((.*?)\);" % (k, kind), hdr, flags=re.S).group(1) for k in ("average", "complete")}
        assert " ".join(decl["complete"].split()) == " ".join(decl["average"].split()), kind
    assert lib.hg_ctx_cluster_complete_rounds.restype == lib.hg_ctx_cluster_average_rounds.restype
    for method in ("cluster_complete", "cluster_complete_dev", "cluster_complete_matrix_dev", "cluster_complete_rounds"):
        assert callable(getattr(hg.Context, method)), method
    import inspect
    for method in ("cluster_complete", "cluster_complete_dev", "cluster_complete_matrix_dev", "cluster_complete_rounds"):
        assert (str(inspect.signature(getattr(hg.Context, method)))
                == str(inspect.signature(getattr(hg.Context, method.replace("complete", "average"))))), method
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NAMES:
        assert "pub fn %s(" % name in integration, name
    # the kernels the header's prose names are in the library
    nmc = subprocess.run(["nm", "-C", hg.LIB_PATH], capture_output=True, text=True).stdout
    named = set(re.findall(r"\bcomplete_[a-z]+_kernel\b", hdr_full))
    assert {"complete_fill_kernel", "complete_mirror_kernel", "complete_best_kernel", "complete_pair_kernel", "complete_rows_kernel",
            "complete_cols_kernel"} <= named
    for k in named:
        assert re.search(r"::%s\(" % k, nmc), k


def test_cluster_help_names_agglomerate_and_keeps_the_general_help(hg, tmp_path):
    general = run(hg, "--help", cwd=str(tmp_path))
    r = run(hg, "cluster", "--help", cwd=str(tmp_path))
    assert (r.returncode, r.stderr) == (0, "")
    assert r.stdout.startswith(general.stdout) and len(r.stdout) > len(general.stdout)
    tail = r.stdout[len(general.stdout):]
    paragraphs = [p for p in tail.split("\n\n") if p.strip()]
    heads = [p.strip().split(":")[0] for p in paragraphs]
    assert heads == ["cluster --hclust average", "cluster --agglomerate average|complete", "cluster --stats <file>"]  # behind --hclust
    para = paragraphs[1]
    assert "complete linkage" in para and "--tree" in para and "--hclust average" in para and "linkage(method=\"complete\")" in para
    assert "--agglomerate" not in general.stdout and "complete linkage" not in general.stdout
    assert os.listdir(str(tmp_path)) == []


WITH_HCLUST = ("error: --agglomerate does not go with --hclust: both choose the clustering on the dense matrix "
               "(--agglomerate average is --hclust average)\n")
WITH_LINKAGE = "error: --agglomerate does not go with --linkage: average and complete linkage are schemes of their own, not ones of --linkage's\n"
WITH_LEVELS = ("error: --levels is not supported with --agglomerate: it cuts the single-linkage tree, not the dendrogram of average or "
               "complete linkage\n")
FAULTS = [
    (("cluster", "--agglomerate", "x"), "error: invalid value 'x' for '--agglomerate' (average | complete)\n"),
    (("cluster", "--agglomerate", "single"), "error: invalid value 'single' for '--agglomerate' (average | complete)\n"),
    (("cluster", "--agglomerate", "complete", "--hclust", "average"), WITH_HCLUST),
    (("cluster", "--hclust", "average", "--agglomerate=average"), WITH_HCLUST),
    (("cluster", "--agglomerate", "complete", "--linkage", "single"), WITH_LINKAGE),
    (("cluster", "--linkage", "greedy", "--agglomerate=complete"), WITH_LINKAGE),
    (("cluster", "--agglomerate", "average", "--linkage", "setcover"), WITH_LINKAGE),
    (("cluster", "--agglomerate", "complete", "--levels", "97,99"), WITH_LEVELS),
    (("cluster", "--agglomerate", "complete", "--tree", "t.tsv", "--levels", "97"), WITH_LEVELS),
    (("cluster", "--agglomerate", "average", "--levels", "97"), WITH_LEVELS),
    # the present messages of the options that do not go with cluster, or with anything but greedy
    (("cluster", "--agglomerate", "complete", "--order", "size"),
     "error: --order needs cluster --linkage greedy: single-linkage components do not depend on the order of the sketches\n"),
    (("cluster", "--agglomerate", "complete", "--shards", "2"), "error: --shards is not supported by cluster: it runs on the first visible GPU\n"),
    (("cluster", "--agglomerate", "complete", "--ani_metric", "containment"),
     "error: --ani_metric containment is not supported by cluster: it is directional (mash | max_containment)\n"),
    # the other subcommands refuse the option with the table's sentence
    (("sketch", "--agglomerate", "complete"), "error: --agglomerate is not supported by sketch: it chooses the agglomerative clustering of cluster\n"),
    (("dist", "--agglomerate", "complete"), "error: --agglomerate is not supported by dist: it chooses the agglomerative clustering of cluster\n"),
    (("search", "--agglomerate", "average"), "error: --agglomerate is not supported by search: it chooses the agglomerative clustering of cluster\n"),
    # --linkage and --hclust keep their value lists
    (("cluster", "--linkage", "complete"), "error: invalid value 'complete' for '--linkage' (single | greedy | setcover)\n"),
    (("cluster", "--hclust", "complete"), "error: invalid value 'complete' for '--hclust' (average)\n"),
]


@pytest.mark.parametrize("args,err", FAULTS, ids=[" ".join(a) for a, _ in FAULTS])
def test_rejected_before_any_device_or_file(hg, tmp_path, args, err):
    # the input does not exist and no device is needed: the option is refused first, and nothing is created
    missing = str(tmp_path / "missing.sketch")
    paths = ("-p", missing) if args[0] in ("cluster", "sketch") else ("-r", missing, "-q", missing)
    r = run(hg, *args, *paths, "-o", "out.tsv", cwd=str(tmp_path))
    assert (r.returncode, r.stderr, r.stdout) == (2, err, "")
    assert os.listdir(str(tmp_path)) == []


@pytest.mark.parametrize("how", ["complete", "average"])
def test_agglomerate_with_tree_is_accepted_up_to_the_required_arguments(hg, tmp_path, how):
    r = run(hg, "cluster", "--agglomerate", how, "--tree", "t.tsv", "--stats", "s.tsv", cwd=str(tmp_path))
    assert (r.returncode, r.stderr) == (2, "error: the following required arguments were not provided: --path --out\n")
    assert os.listdir(str(tmp_path)) == []


def test_the_option_table_stays_within_the_width_of_given():
    src = open(os.path.join(ROOT, "hyper-gen_amd", "csrc", "hg_cli.cpp")).read()
    table = src[src.index("const Option options[] = {"):src.index("const size_t N_OPTIONS")]
    rows = re.findall(r"^    \{\"([a-z_]+)\", ", table, flags=re.M)
    width, = map(int, re.findall(r"std::bitset<(\d+)> given;", src))  # Cli::given, a bit per row
    assert "agglomerate" in rows and len(rows) == len(set(rows)) <= width == 64


# ---- the models on hand-written cases ------------------------------------------------------------------------------
def matrix(n, pairs, fill=0.0):
    a = np.full((n, n), fill, np.float32)
    for (i, j), v in pairs.items():
        a[i, j] = a[j, i] = v
    return a


def same(x, y):
    assert x[5] == y[5]
    for p, q in zip(x[:5], y[:5]):
        assert p.dtype == q.dtype and np.array_equal(p.view(np.uint32), q.view(np.uint32))


def both(a, th):
    """the sequential rule, the round form with the retire and rescan rules and the one that scans every row: identical
    arrays, and the two round forms take the same number of rounds"""
    seq = cp.complete_model(a, th)
    rnd = cp.complete_model_rounds(a, th, with_rounds=True, with_scans=True)
    full = cp.complete_model_rounds(a, th, with_rounds=True, with_scans=True, rescan="all")
    same(seq, rnd)
    same(seq, full)
    assert rnd[6] == full[6] and rnd[7] <= full[7]
    return seq


def test_model_two_items_at_the_threshold_and_below():
    th = 95.0
    rep, cl, into, level, size, nc = both(matrix(2, {(0, 1): 95.0}), th)
    assert (rep.tolist(), cl.tolist(), into.tolist(), size.tolist(), nc) == ([0, 0], [0, 0], [0, 0], [2, 2], 1)
    assert level.tolist() == [0.0, float(np.float32(95.0))]
    below = np.nextafter(np.float32(94.9995), np.float32(0))
    assert cp.milli(below) == cp.th_milli(th) - 1
    rep, cl, into, level, size, nc = both(matrix(2, {(0, 1): below}), th)
    assert (rep.tolist(), cl.tolist(), into.tolist(), level.tolist(), size.tolist(), nc) == ([0, 1], [0, 1], [0, 1], [0.0, 0.0], [1, 1], 2)
    just = np.float32(94.9996)
    assert just < np.float32(95.0) and cp.milli(just) == 95_000
    assert both(matrix(2, {(0, 1): just}), th)[5] == 1  # (below 95 as a float, 95.000 as dist prints it)


def test_model_thresholds_that_merge_nothing_and_everything():
    assert both(matrix(2, {(0, 1): 99.0}), np.nan)[5] == 2 and both(matrix(2, {(0, 1): 100.0}), 100.5)[5] == 2
    assert cp.complete_model_rounds(matrix(2, {(0, 1): 99.0}), np.nan, with_rounds=True)[6] == 0
    assert both(matrix(2, {(0, 1): 100.0}), 100.0)[5] == 1
    # at or below 0 everything merges, pairs of ANI 0 or NaN included
    assert both(matrix(2, {(0, 1): 0.0}), 0.0)[5] == 1 and both(matrix(2, {(0, 1): np.nan}), -1.0)[5] == 1
    a = matrix(4, {(0, 1): np.nan, (2, 3): 50.0})
    rep, cl, into, level, size, nc = both(a, 0.0)
    assert (into.tolist(), nc, size.tolist()) == ([0, 0, 0, 2], 1, [4, 2, 4, 2]) and level.tolist() == [0.0, 0.0, 0.0, 50.0]


def test_model_path_of_three_is_two_clusters_and_joins_only_at_zero():
    a = matrix(3, {(0, 1): 96.0, (1, 2): 96.0, (0, 2): 0.0})
    rep, cl, into, level, size, nc = both(a, 95.0)
    # {0, 1} first (the smaller lower name of two equal pairs); then W({0, 1}, 2) = min(0, 96 000) = 0: below 95
    assert (rep.tolist(), cl.tolist(), into.tolist(), size.tolist(), nc) == ([0, 0, 2], [0, 0, 1], [0, 0, 2], [2, 2, 1], 2)
    assert level.tolist() == [0.0, 96.0, 0.0]
    assert both(a, 0.001)[5] == 2 and both(a, 48.0)[5] == 2  # (average linkage joins the third at 48)
    rep, cl, into, level, size, nc = both(a, 0.0)
    assert (into.tolist(), size.tolist(), nc) == ([0, 0, 0], [3, 2, 3], 1) and level.tolist() == [0.0, 96.0, 0.0]


def test_model_index_ties():
    # all six pairs equal: {0, 1} merges first, then {0 u 1, 2} (lower name 0 beats {2, 3}), then 3
    rep, cl, into, level, size, nc = both(matrix(4, {}, fill=97.0), 95.0)
    assert (into.tolist(), size.tolist(), nc) == ([0, 0, 0, 0], [4, 2, 3, 4], 1) and level.tolist() == [0.0, 97.0, 97.0, 97.0]
    # the higher name decides between {0, 1} and {0, 2}
    a = matrix(3, {(0, 1): 98.0, (0, 2): 98.0, (1, 2): 90.0})
    assert both(a, 97.0)[2].tolist() == [0, 0, 2]


def test_model_two_pairs_of_one_round_get_the_minimum_of_four():
    a = matrix(4, {(0, 1): 99.0, (2, 3): 98.0, (0, 2): 93.0, (0, 3): 91.0, (1, 2): 92.0, (1, 3): 90.5})
    got = cp.complete_model_rounds(a, 90.5, with_rounds=True)
    rep, cl, into, level, size, nc, rounds = got
    assert (into.tolist(), size.tolist(), nc, rounds) == ([0, 0, 0, 2], [4, 2, 4, 2], 1, 3)
    assert level.tolist() == [0.0, 99.0, 90.5, 98.0]  # min(93, 91, 92, 90.5)
    assert cp.complete_model_rounds(a, 90.501)[5] == 2
    both(a, 90.5), both(a, 90.501)
    # the minimum sits in each of the four places in turn
    for low in ((0, 2), (0, 3), (1, 2), (1, 3)):
        b = matrix(4, {(0, 1): 99.0, (2, 3): 98.0, (0, 2): 93.0, (0, 3): 93.0, (1, 2): 93.0, (1, 3): 93.0, low: 90.0})
        assert both(b, 90.0)[3][2] == np.float32(90.0) and both(b, 90.001)[5] == 2


def random_matrix(rng, n, kind):
    if kind == "ties":
        a = rng.integers(0, 4, (n, n)).astype(np.float32)  # milli in {0, 1000, 2000, 3000}: ties everywhere
    elif kind == "coarse":
        a = (rng.integers(0, 4, (n, n)) * 25.0).astype(np.float32)
    else:
        a = rng.uniform(70.0, 100.0, (n, n)).astype(np.float32)
    a = np.triu(a, 1)
    return a + a.T


def test_sequential_model_equals_round_models():
    rng = np.random.default_rng(7)
    merged = skipped = scanned = 0
    for k in range(360):
        n = int(rng.integers(2, 15))
        kind = ("ties", "coarse", "uniform")[k % 3]
        a = random_matrix(rng, n, kind)
        th = {"ties": float(rng.integers(0, 4)), "coarse": float(rng.choice([0.0, 25.0, 40.0, 75.0])),
              "uniform": float(rng.uniform(70.0, 95.0))}[kind]
        got = both(a, th)
        merged += n - got[5]
        r, f = (cp.complete_model_rounds(a, th, with_scans=True, rescan=how)[6] for how in ("invalidated", "all"))
        skipped, scanned = skipped + f - r, scanned + f
        # the lower triangle and the diagonal are not read
        b = a.copy()
        b[np.tril_indices(n)] = np.nan
        same(cp.complete_model(b, th), got)
        same(cp.complete_model_rounds(b, th), got)
    assert merged > 500
    print("row scans skipped by the retire and rescan rules: %d of %d" % (skipped, scanned))
    assert 0 < skipped < scanned  # (the rules are exercised; round 1 always scans every row)
    for n, th in ((40, 80.0), (60, 0.0)):
        a = random_matrix(rng, n, "uniform")
        assert both(a, th)[5] == (1 if th == 0.0 else both(a, th)[5])


def test_every_pair_within_a_cluster_meets_the_threshold_and_no_two_clusters_could_merge():
    rng = np.random.default_rng(21)
    for kind, th in (("uniform", 80.0), ("uniform", 90.0), ("coarse", 50.0), ("ties", 2.0)):
        a = random_matrix(rng, 50, kind)
        rep, cl, into, level, size, nc = cp.complete_model_rounds(a, th)
        m, t = cp.milli_matrix(a), cp.th_milli(th)
        sameset = cl[:, None] == cl[None, :]
        off = ~np.eye(50, dtype=bool)
        assert (m[sameset & off] >= t).all()
        for x in range(nc):
            for y in range(x + 1, nc):
                assert m[np.ix_(cl == x, cl == y)].min() < t
        # the level of a merge is the lowest pair between the two clusters it joined: never above a level inside them
        absorbed = np.flatnonzero(into != np.arange(50))
        assert all(cp.milli(level[b]) >= t for b in absorbed)


def test_partitions_equal_scipy_on_tie_free_matrices():
    hierarchy = pytest.importorskip("scipy.cluster.hierarchy")
    distance = pytest.importorskip("scipy.spatial.distance")
    rng = np.random.default_rng(5)
    for k in range(40):
        n = int(rng.integers(2, 60))
        i, j = np.triu_indices(n, 1)  # tie-free in milli: distinct thousandths, drawn without replacement
        vals = 70_000 + rng.choice(30_001, i.size, replace=False)
        a = np.zeros((n, n), np.float32)
        a[i, j] = a[j, i] = (vals / 1000.0).astype(np.float32)
        assert np.array_equal(cp.milli_matrix(a)[i, j], vals)
        th = float(rng.uniform(72.0, 98.0))
        d = 100_000 - cp.milli_matrix(a)
        np.fill_diagonal(d, 0)
        z = hierarchy.linkage(distance.squareform(d.astype(np.float64), checks=False), method="complete")
        want = hierarchy.fcluster(z, t=100_000 - cp.th_milli(th), criterion="distance")  # cophenetic distance <= t: W >= th_milli
        cl = cp.complete_model_rounds(a, th)[1]
        assert np.array_equal(cl[:, None] == cl[None, :], want[:, None] == want[None, :]), (k, n, th)


def test_merge_order_puts_children_before_parents():
    rng = np.random.default_rng(3)
    for kind in ("ties", "uniform", "coarse"):
        a = random_matrix(rng, 60, kind)
        rep, cl, into, level, size, nc = cp.complete_model_rounds(a, 0.0)
        assert nc == 1
        order = cp.merge_order(into, level, size)
        assert len(order) == 59
        built = {i: 1 for i in range(60)}  # name -> current size, replaying the merges in the listed order
        gone = set()
        last = np.inf
        for b in order:
            assert b not in gone and int(into[b]) not in gone and into[b] < b
            built[int(into[b])] += built[b]
            assert built[int(into[b])] == size[b]  # every merge below this one has been listed: children come first
            gone.add(b)
            assert level[b] <= last  # levels never rise towards the root
            last = level[b]
