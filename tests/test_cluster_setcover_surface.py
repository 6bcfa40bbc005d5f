"""Greedy set-cover clustering (hg_cluster_setcover*, `hyper-gen cluster --linkage setcover`), the parts that need no GPU:
the C ABI's declarations and exports, the command line's surface (help, what it rejects before a device is opened or a
file read), and the CPU model of tests/cluster_setcover_ref.py on hand-written cases."""
import os
import re
import subprocess

import numpy as np
import pytest

import cluster_greedy_ref as gr
import cluster_setcover_ref as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("hg_cluster_setcover_hits_dev", "hg_cluster_setcover_dev", "hg_cluster_setcover", "hg_ctx_cluster_setcover_rounds")


@pytest.fixture(scope="module")
def hg():
    import hypergen_amd
    hypergen_amd.lib()
    return hypergen_amd


def run(hg, *args):
    return subprocess.run([hg.CLI_PATH] + list(args), capture_output=True, text=True, timeout=60)


def test_setcover_symbols_declared_and_exported(hg):
    hdr_full = open(os.path.join(ROOT, "include", "hypergen.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr_full, flags=re.S)
    nm = subprocess.run(["nm", "-D", "--defined-only", hg.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r"\bT (hg_\w+)", nm))
    for name in NAMES:
        assert re.search(r"\b(hg_status|uint64_t) %s\(" % name, hdr), name
        assert name in exported, name
        assert name in hg.EXPORTS, name
    assert '"setcover_rounds"' in hdr_full
    for method in ("cluster_setcover", "cluster_setcover_dev", "cluster_setcover_hits_dev", "cluster_setcover_rounds"):
        assert callable(getattr(hg.Context, method)), method


def test_help_names_the_linkage(hg):
    r = run(hg, "--help")
    assert r.returncode == 0
    assert "--linkage single|greedy|setcover" in r.stdout


REJECTED = [
    (("cluster", "--linkage", "setcover", "--order", "size"), "--order"),
    (("cluster", "--linkage", "setcover", "--order", "file"), "--order"),
    (("cluster", "--linkage", "setcover", "--tree", "t.tsv"), "--tree"),
    (("cluster", "--linkage", "setcover", "--levels", "97,99"), "--levels"),
    (("cluster", "--linkage", "setcover", "--ani_metric", "containment"), "--ani_metric"),
    (("cluster", "--linkage", "setcover", "--shards", "2"), "--shards"),
    (("dist", "--linkage", "setcover"), "--linkage"),
    (("cluster", "--linkage", "cover"), "--linkage"),
]


@pytest.mark.parametrize("args,flag", REJECTED, ids=[" ".join(a) for a, _ in REJECTED])
def test_rejected_before_any_device_or_file(hg, tmp_path, args, flag):
    # the input does not exist and no device is needed: the option is refused first
    missing, out = str(tmp_path / "missing.sketch"), tmp_path / "out.tsv"
    paths = ("-p", missing) if args[0] in ("cluster", "sketch") else ("-r", missing, "-q", missing)
    r = run(hg, *args, *paths, "-o", str(out))
    assert r.returncode != 0
    assert flag in r.stderr, r.stderr
    assert "missing.sketch" not in r.stderr  # (nothing tried to open it)
    assert not out.exists()


# ---- the model on hand-written cases ---------------------------------------------------------------------------------
def edges(*stars):
    """(centre, leaves, ani) ... -> a, b, ani"""
    a, b, v = [], [], []
    for centre, leaves, ani in stars:
        for leaf in leaves:
            a.append(centre), b.append(leaf), v.append(ani)
    return a, b, v


def check(got, rep, count, ani=None):
    assert got[0].tolist() == rep and got[3] == count
    assert got[0].dtype == np.uint32 and got[1].dtype == np.uint32 and got[2].dtype == np.float32
    roots = sorted(set(rep))
    assert len(roots) == count and got[1].tolist() == [roots.index(r) for r in rep]
    if ani is None:
        ani = [100.0 if r == i else 97.0 for i, r in enumerate(rep)]
    assert got[2].tolist() == [float(np.float32(x)) for x in ani]


def test_model_chain_of_three_is_one_cluster_around_the_middle():
    check(sc.setcover_model(3, [0, 1], [1, 2], 97.0, 95.0), [1, 1, 1], 1)
    assert gr.greedy_model(3, [0, 1], [1, 2], 97.0, 95.0)[3] == 2


def test_model_four_cycle():
    # every degree is 2: 0 is chosen, takes 1 and 3; 2 is left alone
    check(sc.setcover_model(4, [0, 1, 2, 3], [1, 2, 3, 0], 97.0, 95.0), [0, 0, 2, 0], 2)


def test_model_degrees_are_recounted():
    # static degrees: 0 has 5, 6 has 4, 7 and 8 have 3.  Once 0 has taken 3, 4 and 5, node 6 is left with 7 alone, and
    # 7 (12, 13 and 6) and 8 are chosen before it: a rule that does not recount would make 6 a representative
    a, b, v = edges((0, [1, 2, 3, 4, 5], 97.0), (6, [3, 4, 5, 7], 97.0), (8, [9, 10, 11], 97.0), (7, [12, 13], 97.0))
    check(sc.setcover_model(14, a, b, v, 95.0), [0, 0, 0, 0, 0, 0, 7, 7, 8, 8, 8, 8, 7, 7], 3)


def test_model_two_stars_sharing_a_leaf():
    # leaf 6 belongs to the larger star (0, six leaves) whatever the ANI: 10 has five
    a, b, v = edges((0, [1, 2, 3, 4, 5, 6], 96.0), (10, [6], 99.0), (10, [11, 12, 13, 14], 96.0))
    got = sc.setcover_model(15, a, b, v, 95.0)
    rep = [0, 0, 0, 0, 0, 0, 0, 7, 8, 9, 10, 10, 10, 10, 10]
    check(got, rep, 5, [100.0 if r == i else 96.0 for i, r in enumerate(rep)])
    assert got[2][6] == np.float32(96.0)


def test_model_star_on_the_last_index():
    n = 1000
    leaves = np.arange(n - 1)
    got = sc.setcover_model(n, np.full(n - 1, n - 1), leaves, 97.0, 95.0)
    check(got, [n - 1] * n, 1)
    assert gr.greedy_model(n, np.full(n - 1, n - 1), leaves, 97.0, 95.0)[3] == n - 1


def test_model_orientation_duplicates_self_pairs_and_threshold_side():
    th = np.float32(95.0)
    below = np.nextafter(th, np.float32(0))
    want = sc.setcover_model(3, [0, 1], [1, 2], [96.0, 97.0], 95.0)
    check(want, [1, 1, 1], 1, [96.0, 100.0, 97.0])
    # reversed orientation; a duplicate with a lower ANI (both records of the pair, so that every pair is given twice);
    # self-pairs
    for a, b, v in (([1, 2], [0, 1], [96.0, 97.0]),
                    ([0, 1, 1, 2], [1, 2, 0, 1], [96.0, 97.0, 95.5, 96.5]),
                    ([0, 1, 0, 1, 2], [1, 2, 0, 1, 2], [96.0, 97.0, 100.0, 100.0, 100.0])):
        got = sc.setcover_model(3, a, b, v, 95.0)
        assert all(np.array_equal(x, y) for x, y in zip(got[:3], want[:3])) and got[3] == want[3]
    # degrees count records.  The path 3 - 0 - 1 - 2 - 4: 0, 1 and 2 have two records each, 0 is chosen, then 2.  With
    # 3 - 0 given twice 0 has three: the same.  With 1 - 2 given twice 1 and 2 have three: 1 is chosen, 3 and 4 stay alone.
    check(sc.setcover_model(5, [3, 0, 1, 2], [0, 1, 2, 4], 97.0, 95.0), [0, 0, 2, 0, 2], 2)
    check(sc.setcover_model(5, [3, 3, 0, 1, 2], [0, 0, 1, 2, 4], 97.0, 95.0), [0, 0, 2, 0, 2], 2)
    check(sc.setcover_model(5, [3, 0, 1, 1, 2], [0, 1, 2, 2, 4], 97.0, 95.0), [1, 1, 1, 3, 4], 3)
    # the threshold: at th the pair counts, one ulp below it does not
    a, b, v = [0, 2], [1, 3], [th, below]
    check(sc.setcover_model(4, a, b, v, float(th)), [0, 0, 2, 3], 3, [100.0, th, 100.0, 100.0])
    check(sc.setcover_model(4, a, b, v, float(below)), [0, 0, 2, 2], 2, [100.0, th, 100.0, below])
    assert sc.setcover_model(2, [0], [1], [np.nan], 95.0)[3] == 2  # NaN never counts
    with pytest.raises(ValueError):
        sc.setcover_model(3, [0], [3], [99.0], 95.0)
    with pytest.raises(ValueError):
        sc.setcover_model(3, [0], [3], [10.0], 95.0)  # below the threshold too
    got = sc.setcover_model(0, [], [], [], 95.0)
    assert got[3] == 0 and got[0].size == 0


def test_model_every_pair_twice_resolves_like_every_pair_once():
    rng = np.random.default_rng(5)
    n, m = 300, 900
    a, b = rng.integers(0, n, m), rng.integers(0, n, m)
    pairs = np.unique(np.stack([np.minimum(a, b), np.maximum(a, b)], 1), axis=0)  # each pair once
    a, b = pairs[:, 0], pairs[:, 1]
    v = rng.uniform(90.0, 100.0, a.size).astype(np.float32)
    once = sc.setcover_model(n, a, b, v, 95.0)
    twice = sc.setcover_model(n, np.concatenate([a, b]), np.concatenate([b, a]), np.concatenate([v, v]), 95.0)
    assert all(np.array_equal(x, y) for x, y in zip(once[:3], twice[:3])) and once[3] == twice[3]
    assert 1 < once[3] < n


def test_model_on_a_matrix_matches_the_edge_list_form_and_keeps_both_invariants():
    rng = np.random.default_rng(3)
    a = rng.uniform(90.0, 100.0, (40, 40)).astype(np.float32)
    a = np.maximum(a, a.T)
    got = sc.setcover_model_matrix(a, 97.0)
    i, j = np.nonzero(np.triu(np.ones_like(a, bool), 1))
    want = sc.setcover_model(40, j, i, a[i, j], 97.0)  # every pair, reversed orientation
    assert all(np.array_equal(x, y) for x, y in zip(got[:3], want[:3])) and got[3] == want[3]
    reps = np.flatnonzero(got[0] == np.arange(40))
    assert (a[np.ix_(reps, reps)][~np.eye(reps.size, dtype=bool)] < np.float32(97.0)).all()
    m = np.flatnonzero(got[0] != np.arange(40))
    assert (a[got[0][m], m] >= np.float32(97.0)).all() and np.array_equal(a[got[0][m], m], got[2][m])
