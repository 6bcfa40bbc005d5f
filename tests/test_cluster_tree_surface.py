"""The single-linkage tree (hg_cluster_tree*, `hyper-gen cluster --tree / --levels`), the parts that need no GPU: the C ABI's
declarations and exports, the command line's surface (help, what it rejects before a device is opened or a file read),
and the CPU model of tests/cluster_tree_ref.py on hand-written cases and against a transitive-closure count."""
import os
import re
import subprocess

import numpy as np
import pytest

import cluster_tree_ref as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("hg_cluster_tree_hits_dev", "hg_cluster_tree_dev", "hg_cluster_tree", "hg_ctx_cluster_tree_rounds")


@pytest.fixture(scope="module")
def hg():
    import hypergen_amd
    hypergen_amd.lib()
    return hypergen_amd


def run(hg, *args):
    return subprocess.run([hg.CLI_PATH] + list(args), capture_output=True, text=True, timeout=60)


def test_tree_symbols_declared_and_exported(hg):
    hdr_full = open(os.path.join(ROOT, "include", "hypergen.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr_full, flags=re.S)
    nm = subprocess.run(["nm", "-D", "--defined-only", hg.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r"\bT (hg_\w+)", nm))
    for name in NAMES:
        assert re.search(r"\b(hg_status|uint64_t)\s+%s\(" % name, hdr), name
        assert name in exported, name
        assert name in hg.EXPORTS, name
    assert '"tree_rounds"' in hdr_full
    for method in ("cluster_tree", "cluster_tree_dev", "cluster_tree_hits_dev", "cluster_tree_rounds"):
        assert callable(getattr(hg.Context, method)), method


def test_tree_kernels_are_named_as_a_family(hg):
    nm = subprocess.run(["nm", "-C", hg.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert set(re.findall(r"\b(tree_\w+_kernel)\b", nm)) == {"tree_init_kernel", "tree_best_ani_kernel", "tree_best_pair_kernel",
                                                              "tree_select_kernel", "tree_hook_kernel", "tree_compress_kernel"}


def test_help_names_tree_and_levels(hg):
    r = run(hg, "--help")
    assert r.returncode == 0
    assert "--tree" in r.stdout and "--levels" in r.stdout
    assert "--linkage single|greedy" in r.stdout


REJECTED = [
    (("cluster", "--linkage", "greedy", "--tree", "t.tsv"), "--tree"),
    (("cluster", "--linkage", "greedy", "--levels", "97,99"), "--levels"),
    (("cluster", "--tree", "t.tsv", "--shards", "2"), "--tree"),
    (("cluster", "--levels", "97", "--shards", "2"), "--levels"),
    (("dist", "--tree", "t.tsv"), "--tree"),
    (("search", "--tree", "t.tsv"), "--tree"),
    (("sketch", "--tree", "t.tsv"), "--tree"),
    (("dist", "--levels", "97"), "--levels"),
    (("search", "--levels", "97"), "--levels"),
    (("sketch", "--levels", "97"), "--levels"),
    (("cluster", "--levels", ""), "--levels"),
    (("cluster", "--levels", "97,,99"), "--levels"),
    (("cluster", "--levels", "97,"), "--levels"),
    (("cluster", "--levels", "97,abc"), "--levels"),
    (("cluster", "--levels", "97;99"), "--levels"),
    (("cluster", "--levels", "nan"), "--levels"),
    (("cluster", "--levels", "99,97"), "--levels"),
    (("cluster", "--levels", "97,97"), "--levels"),
    (("cluster", "--levels", "96,96.5,97,97.5,98,98.5,99,99.5,99.9"), "--levels"),
    (("cluster", "--levels", "95,97"), "--levels"),            # not above the default -a 95
    (("cluster", "-a", "97", "--levels", "96,98"), "--levels"),  # not above the given -a
    (("cluster", "--levels", "98,99", "-a", "98"), "--levels"),  # -a behind the flag
]


@pytest.mark.parametrize("args,flag", REJECTED, ids=[" ".join(a) for a, _ in REJECTED])
def test_rejected_before_any_device_or_file(hg, tmp_path, args, flag):
    # the input does not exist and no device is needed: the option is refused first
    missing, out = str(tmp_path / "missing.sketch"), tmp_path / "out.tsv"
    paths = ("-p", missing) if args[0] in ("cluster", "sketch") else ("-r", missing, "-q", missing)
    r = subprocess.run([hg.CLI_PATH] + list(args) + list(paths) + ["-o", str(out)], capture_output=True, text=True, timeout=60,
                       cwd=str(tmp_path))
    assert r.returncode != 0
    assert flag in r.stderr, r.stderr
    assert "missing.sketch" not in r.stderr  # (nothing tried to open it)
    assert not out.exists() and not (tmp_path / "t.tsv").exists()


# ---- the model on hand-written cases ---------------------------------------------------------------------------------
def edges(t):
    return list(zip(t["ref_idx"].tolist(), t["qry_idx"].tolist(), t["ani"].tolist()))


def test_model_triangle_loses_its_weakest_edge():
    t, rep, cl, nc = tr.tree_model(3, [0, 1, 0], [1, 2, 2], [97.0, 99.0, 96.0], 95.0)
    assert edges(t) == [(1, 2, 99.0), (0, 1, 97.0)]
    assert rep.tolist() == [0, 0, 0] and cl.tolist() == [0, 0, 0] and nc == 1
    assert t.dtype == tr.TREE_DTYPE and rep.dtype == np.uint32 and cl.dtype == np.uint32


def test_model_ties_go_to_the_smaller_lo_then_hi():
    i, j = np.triu_indices(64, 1)
    t, rep, cl, nc = tr.tree_model(64, j, i, np.float32(97.0), 95.0)  # K64, every ANI equal, reversed orientation
    assert edges(t) == [(0, k, 97.0) for k in range(1, 64)]
    assert nc == 1
    k = np.arange(1000)
    t, _, _, nc = tr.tree_model(1000, k, (k + 1) % 1000, np.float32(98.0), 95.0)  # a ring
    want = sorted([(min(x, (x + 1) % 1000), max(x, (x + 1) % 1000)) for x in range(1000)])
    want.remove((998, 999))
    assert [(a, b) for a, b, _ in edges(t)] == want and nc == 1


def test_model_orientation_duplicates_self_pairs_and_threshold_side():
    th = np.float32(95.0)
    below = np.nextafter(th, np.float32(0))
    # (1, 0) reversed and given with two values: the strongest decides; an exact duplicate; a self-pair; one edge at the
    # threshold, one an ulp below
    a, b, v = [1, 0, 0, 2, 3, 2], [0, 1, 1, 2, 0, 4], [96.0, 97.0, 97.0, 100.0, below, th]
    t, rep, cl, nc = tr.tree_model(5, a, b, v, float(th))
    assert edges(t) == [(0, 1, 97.0), (2, 4, 95.0)] and rep.tolist() == [0, 0, 2, 3, 2] and cl.tolist() == [0, 0, 1, 2, 1] and nc == 3
    t, rep, cl, nc = tr.tree_model(5, a, b, v, float(below))
    assert edges(t) == [(0, 1, 97.0), (2, 4, 95.0), (0, 3, float(below))] and rep.tolist() == [0, 0, 2, 0, 2] and nc == 2
    # NaN never counts; -0 and +0 are one value, and negative ANIs order as floats
    t, _, _, nc = tr.tree_model(4, [0, 1, 2, 0], [1, 2, 3, 3], [np.nan, -0.0, -1.5, 0.0], -2.0)
    assert [(x, y) for x, y, _ in edges(t)] == [(0, 3), (1, 2), (2, 3)] and nc == 1
    assert t["ani"].view(np.uint32).tolist() == np.array([0.0, 0.0, -1.5], np.float32).view(np.uint32).tolist()
    with pytest.raises(IndexError):
        tr.tree_model(3, [0], [3], [10.0], 95.0)  # below the threshold too
    t, rep, cl, nc = tr.tree_model(0, [], [], [], 95.0)
    assert t.size == 0 and rep.size == 0 and cl.size == 0 and nc == 0
    t, rep, cl, nc = tr.tree_model(1, [0], [0], [100.0], 95.0)
    assert t.size == 0 and rep.tolist() == [0] and cl.tolist() == [0] and nc == 1


def test_model_on_a_matrix_matches_the_edge_list_form():
    rng = np.random.default_rng(3)
    a = rng.choice(np.linspace(90.0, 100.0, 21).astype(np.float32), (40, 40))
    a = np.maximum(a, a.T)
    got = tr.tree_model_matrix(a, 97.0)
    i, j = np.nonzero(np.triu(np.ones_like(a, bool), 1))
    p = rng.permutation(i.size)
    want = tr.tree_model(40, j[p], i[p], a[i, j][p], 97.0)  # every pair, reversed orientation, shuffled
    assert got[0].tobytes() == want[0].tobytes()
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]) and got[3] == want[3]
    assert got[0].size == 40 - got[3]


def test_model_cut_property_against_transitive_closure():
    rng = np.random.default_rng(5)
    n, m = 300, 600
    a, b = rng.integers(0, n, m), rng.integers(0, n, m)
    v = rng.choice(np.linspace(90.0, 100.0, 41).astype(np.float32), m)
    floor = 92.0
    t, rep, cl, nc = tr.tree_model(n, a, b, v, floor)
    assert nc == tr.closure_count(n, a, b, v, floor) and t.size == n - nc
    assert (np.diff(t["ani"]) <= 0).all()
    one = np.float32(96.0)
    for level in (floor, 94.25, float(one), float(np.nextafter(one, np.float32(200))), 99.75, 100.0, 101.0):
        got = tr.cut(n, t, level)
        want = tr.components(n, a, b, v, level)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2], level
        assert got[2] == tr.closure_count(n, a, b, v, level), level
    assert tr.cut(n, t, float(one))[2] < tr.cut(n, t, float(np.nextafter(one, np.float32(200))))[2]


def test_model_random_list_of_the_gpu_tests():
    rng = np.random.default_rng(11)
    n, m = 20_000, 100_000
    a, b = rng.integers(0, n, m, dtype=np.uint32), rng.integers(0, n, m, dtype=np.uint32)
    v = rng.choice(np.linspace(90.0, 100.0, 41).astype(np.float32), m)
    t, rep, cl, nc = tr.tree_model(n, a, b, v, 95.0)
    kept = tr.counting_edges(n, a, b, v, 95.0)[0].size
    assert 1 < nc < n and t.size == n - nc < kept
    p = rng.permutation(m)
    assert tr.tree_model(n, b[p], a[p], v[p], 95.0)[0].tobytes() == t.tobytes()  # hit order and orientation do not show
