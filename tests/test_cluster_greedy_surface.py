"""Greedy representative clustering (hg_cluster_greedy*, `hyper-gen cluster --linkage greedy`), the parts that need no GPU:
the C ABI's declarations and exports, the command line's surface (help, what it rejects before a device is opened or a
file read), and the CPU model of tests/cluster_greedy_ref.py on hand-written cases."""
import os
import re
import subprocess

import numpy as np
import pytest

import cluster_greedy_ref as gr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("hg_cluster_greedy_hits_dev", "hg_cluster_greedy_dev", "hg_cluster_greedy", "hg_ctx_cluster_greedy_rounds")


@pytest.fixture(scope="module")
def hg():
    import hypergen_amd
    hypergen_amd.lib()
    return hypergen_amd


def run(hg, *args):
    return subprocess.run([hg.CLI_PATH] + list(args), capture_output=True, text=True, timeout=60)


def test_greedy_symbols_declared_and_exported(hg):
    hdr_full = open(os.path.join(ROOT, "include", "hypergen.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr_full, flags=re.S)
    nm = subprocess.run(["nm", "-D", "--defined-only", hg.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r"\bT (hg_\w+)", nm))
    for name in NAMES:
        assert re.search(r"\b(hg_status|uint64_t) %s\(" % name, hdr), name
        assert name in exported, name
        assert name in hg.EXPORTS, name
    assert '"greedy_rounds"' in hdr_full
    for method in ("cluster_greedy", "cluster_greedy_dev", "cluster_greedy_hits_dev", "cluster_greedy_rounds"):
        assert callable(getattr(hg.Context, method)), method


def test_help_names_linkage_and_order(hg):
    r = run(hg, "--help")
    assert r.returncode == 0
    assert "--linkage single|greedy" in r.stdout
    assert "--order file|size" in r.stdout
    assert "<sketch|dist|search|cluster>" in run(hg).stderr


REJECTED = [
    (("cluster", "--linkage", "complete"), "--linkage"),
    (("cluster", "--linkage", "greedy", "--order", "length"), "--order"),
    (("cluster", "--order", "size"), "--order"),
    (("cluster", "--linkage", "single", "--order", "size"), "--order"),
    (("dist", "--linkage", "greedy"), "--linkage"),
    (("search", "--linkage", "single"), "--linkage"),
    (("sketch", "--linkage", "greedy"), "--linkage"),
    (("cluster", "--linkage", "greedy", "--shards", "2"), "--shards"),
    (("cluster", "--linkage", "greedy", "--ani_metric", "containment"), "--ani_metric"),
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
def check(got, rep, cluster, ani, count):
    assert got[0].tolist() == rep and got[1].tolist() == cluster and got[3] == count
    assert got[0].dtype == np.uint32 and got[1].dtype == np.uint32 and got[2].dtype == np.float32
    assert got[2].tolist() == [float(np.float32(x)) for x in ani]


def test_model_chain_of_three_is_two_clusters():
    # ani(0, 1) and ani(1, 2) at the threshold or above, ani(0, 2) below: single linkage makes one component of it
    check(gr.greedy_model(3, [0, 1], [1, 2], [96.0, 97.0], 95.0), [0, 0, 2], [0, 0, 1], [100.0, 96.0, 100.0], 2)
    check(gr.greedy_model(3, [0, 1, 0], [1, 2, 2], [96.0, 97.0, 94.0], 95.0), [0, 0, 2], [0, 0, 1], [100.0, 96.0, 100.0], 2)


def test_model_a_member_does_not_cover():
    # 1 is a member of 0; 2 is within the threshold of 1 only -> a representative; 3 joins 2, not the member 1
    check(gr.greedy_model(4, [0, 1, 1, 2], [1, 2, 3, 3], [99.0, 99.0, 99.5, 96.0], 95.0),
          [0, 0, 2, 2], [0, 0, 1, 1], [100.0, 99.0, 100.0, 96.0], 2)


def test_model_tie_goes_to_the_smallest_index():
    # representatives 0, 1, 2 (no edges among them); 3 is equally close to 1 and 2, and closer to them than to 0
    check(gr.greedy_model(4, [2, 1, 0], [3, 3, 3], [98.0, 98.0, 97.0], 95.0), [0, 1, 2, 1], [0, 1, 2, 1], [100.0, 100.0, 100.0, 98.0], 3)


def test_model_a_later_better_representative_is_not_taken():
    # 1 joins 0 at 96; 2 is a representative (nothing joins it to 0) and lies at 99 of 1: 1 stays with 0
    check(gr.greedy_model(3, [0, 1], [1, 2], [96.0, 99.0], 95.0), [0, 0, 2], [0, 0, 1], [100.0, 96.0, 100.0], 2)


def test_model_orientation_duplicates_self_pairs_and_threshold_side():
    th = np.float32(95.0)
    below = np.nextafter(th, np.float32(0))
    # (1, 0) reversed, given twice with two values: the highest wins; a self-pair; one edge at the threshold, one an ulp below
    a, b, v = [1, 0, 2, 3, 2], [0, 1, 2, 0, 4], [96.0, 97.0, 100.0, below, th]
    check(gr.greedy_model(5, a, b, v, float(th)), [0, 0, 2, 3, 2], [0, 0, 1, 2, 1], [100.0, 97.0, 100.0, 100.0, 95.0], 3)
    check(gr.greedy_model(5, a, b, v, float(below)), [0, 0, 2, 0, 2], [0, 0, 1, 0, 1], [100.0, 97.0, 100.0, below, 95.0], 2)
    with pytest.raises(ValueError):
        gr.greedy_model(3, [0], [3], [99.0], 95.0)
    assert gr.greedy_model(0, [], [], [], 95.0)[3] == 0


def test_model_on_a_matrix_matches_the_edge_list_form():
    rng = np.random.default_rng(3)
    a = rng.uniform(90.0, 100.0, (40, 40)).astype(np.float32)
    a = np.maximum(a, a.T)
    got = gr.greedy_model_matrix(a, 97.0)
    i, j = np.nonzero(np.triu(np.ones_like(a, bool), 1))
    want = gr.greedy_model(40, j, i, a[i, j], 97.0)  # every pair, reversed orientation
    assert all(np.array_equal(x, y) for x, y in zip(got[:3], want[:3])) and got[3] == want[3]
    reps = np.flatnonzero(got[0] == np.arange(40))
    assert (a[np.ix_(reps, reps)][~np.eye(reps.size, dtype=bool)] < np.float32(97.0)).all()
    m = np.flatnonzero(got[0] != np.arange(40))
    assert (a[got[0][m], m] >= np.float32(97.0)).all() and np.array_equal(a[got[0][m], m], got[2][m])
