"""Cluster statistics (hg_cluster_stats*, `hyper-gen cluster --stats`), the parts that need no GPU: the C ABI's declarations,
exports and record layouts, the command line's surface (cluster --help, what it rejects before a device is opened or a file
read) and the CPU model of tests/cluster_stats_ref.py on hand-written cases."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import cluster_stats_ref as st

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("hg_cluster_stats_matrix_dev", "hg_cluster_stats_dev", "hg_cluster_stats")
NONE = st.NONE


@pytest.fixture(scope="module")
def hg():
    import hypergen_amd
    hypergen_amd.lib()
    return hypergen_amd


def run(hg, *args, cwd=None):
    return subprocess.run([hg.CLI_PATH] + list(args), capture_output=True, text=True, timeout=60, cwd=cwd)


def test_stats_symbols_declared_exported_and_bound(hg):
    hdr_full = open(os.path.join(ROOT, "include", "hypergen.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr_full, flags=re.S)
    nm = subprocess.run(["nm", "-D", "--defined-only", hg.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r"\bT (hg_\w+)", nm))
    for name in NAMES:
        assert re.search(r"\bhg_status %s\(" % name, hdr), name
        assert name in exported, name
        assert name in hg.EXPORTS, name
        assert getattr(hg.lib(), name).argtypes is not None, name
    assert re.search(r"#define HG_STATS_NONE 0xFFFFFFFFu\b", hdr) and hg.STATS_NONE == 0xFFFFFFFF == NONE
    assert '"stats_block_rows"' in hdr_full
    assert len(hg.lib().hg_cluster_stats_matrix_dev.argtypes) == 7
    assert len(hg.lib().hg_cluster_stats_dev.argtypes) == len(hg.lib().hg_cluster_stats.argtypes) == 10
    for method in ("cluster_stats", "cluster_stats_dev", "cluster_stats_matrix_dev"):
        assert callable(getattr(hg.Context, method)), method
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NAMES:
        assert "pub fn %s(" % name in integration, name


def test_record_layouts(hg):
    node = [("within_sum", 0, 8), ("within_min", 8, 4), ("within_min_idx", 12, 4), ("outside_max", 16, 4), ("outside_max_idx", 20, 4)]
    stat = [("within_sum", 0, 8), ("size", 8, 4), ("first", 12, 4), ("medoid", 16, 4), ("within_min", 20, 4), ("within_min_a", 24, 4),
            ("within_min_b", 28, 4), ("outside_max", 32, 4), ("outside_member", 36, 4), ("outside_idx", 40, 4), ("reserved", 44, 4)]
    assert ctypes.sizeof(hg.NodeStat) == 24 and ctypes.sizeof(hg.ClusterStat) == 48
    for cls, dtype, model, fields in ((hg.NodeStat, hg.NODE_STAT_DTYPE, st.NODE_DTYPE, node),
                                      (hg.ClusterStat, hg.CLUSTER_STAT_DTYPE, st.CLUSTER_DTYPE, stat)):
        assert [f[0] for f in cls._fields_] == [f[0] for f in fields]
        for name, off, size in fields:
            assert (getattr(cls, name).offset, getattr(cls, name).size) == (off, size), name
            assert (dtype.fields[name][1], dtype.fields[name][0].itemsize) == (off, size), name
        assert dtype == model and dtype.itemsize == ctypes.sizeof(cls)
    # the header declares the fields in this order
    hdr = open(os.path.join(ROOT, "include", "hypergen.h")).read()
    for typ, fields in (("hg_node_stat", node), ("hg_cluster_stat", stat)):
        body = re.search(r"typedef struct \{([^}]*)\} %s;" % typ, hdr).group(1)
        assert re.findall(r"\b([a-z_]+)\s*[,;]", body) == [f[0] for f in fields]


def test_cluster_help_names_stats_and_the_general_help_does_not(hg, tmp_path):
    general = run(hg, "--help", cwd=str(tmp_path))
    r = run(hg, "cluster", "--help", cwd=str(tmp_path))
    assert (r.returncode, r.stderr) == (0, "")
    assert r.stdout.startswith(general.stdout)
    tail = r.stdout[len(general.stdout):]
    assert "--stats <file>" in tail and tail.index("--hclust average") < tail.index("--stats")
    assert "--stats" not in general.stdout
    assert os.listdir(str(tmp_path)) == []


FAULTS = [
    (("cluster", "--stats", ""), "error: invalid value '' for '--stats' (a file name)\n"),
    (("cluster", "--stats="), "error: invalid value '' for '--stats' (a file name)\n"),
    (("sketch", "--stats", "f"), "error: --stats is not supported by sketch: it describes the clusters of cluster\n"),
    (("dist", "--stats", "f"), "error: --stats is not supported by dist: it describes the clusters of cluster\n"),
    (("search", "--stats", "f"), "error: --stats is not supported by search: it describes the clusters of cluster\n"),
    (("cluster", "--stats", "f", "--shards", "2"), "error: --stats is not supported with --shards: cluster runs on the first visible GPU\n"),
]


@pytest.mark.parametrize("args,err", FAULTS, ids=[" ".join(a) for a, _ in FAULTS])
def test_rejected_before_any_device_or_file(hg, tmp_path, args, err):
    missing = str(tmp_path / "missing.sketch")
    paths = ("-p", missing) if args[0] in ("cluster", "sketch") else ("-r", missing, "-q", missing)
    r = run(hg, *args, *paths, "-o", "out.tsv", cwd=str(tmp_path))
    assert (r.returncode, r.stderr, r.stdout) == (2, err, "")
    assert os.listdir(str(tmp_path)) == []


@pytest.mark.parametrize("more", [(), ("--linkage", "greedy", "--order", "size"), ("--linkage", "setcover"), ("--hclust", "average"),
                                  ("--tree", "t.tsv", "--levels", "97,99")], ids=lambda m: " ".join(m) or "single")
def test_stats_goes_with_every_scheme_up_to_the_required_arguments(hg, tmp_path, more):
    r = run(hg, "cluster", "--stats", "f", *more, cwd=str(tmp_path))
    assert (r.returncode, r.stderr, r.stdout) == (2, "error: the following required arguments were not provided: --path --out\n", "")
    assert os.listdir(str(tmp_path)) == []


# ---- the model on hand-written cases ---------------------------------------------------------------------------------
def matrix(n, pairs, fill=0.0):
    a = np.full((n, n), fill, np.float32)
    for (i, j), v in pairs.items():
        a[i, j] = a[j, i] = v
    return a


def rec(r):
    return tuple(int(r[k]) for k in r.dtype.names)


def test_model_path_of_three_in_one_cluster_shows_the_chaining():
    a = matrix(3, {(0, 1): 96.0, (1, 2): 96.0, (0, 2): 0.0})
    nodes, stats = st.stats_model(a, [0, 0, 0], 1)
    assert [rec(x) for x in nodes] == [(96_000, 0, 2, NONE, NONE), (192_000, 96_000, 0, NONE, NONE), (96_000, 0, 0, NONE, NONE)]
    # within_sum, size, first, medoid, within_min, _a, _b, outside_max, outside_member, outside_idx, reserved
    assert rec(stats[0]) == (384_000, 3, 0, 1, 0, 0, 2, NONE, NONE, NONE, 0)
    assert st.mean_within(stats[0]["within_sum"], 3) == np.float32(64.0)
    assert st.stats_lines(stats, [0, 0, 0], ["a", "b", "c"]) == "0\t3\tb\t64.000\t0.000\ta\tc\tNA\tNA\tNA\tNA\n"
    assert st.not_separated(stats) == 0
    # as average linkage splits it: {0, 1} and {2}
    nodes, stats = st.stats_model(a, [0, 0, 1], 2)
    assert [rec(x) for x in nodes] == [(96_000, 96_000, 1, 0, 2), (96_000, 96_000, 0, 96_000, 2), (0, NONE, NONE, 96_000, 1)]
    assert rec(stats[0]) == (192_000, 2, 0, 0, 96_000, 0, 1, 96_000, 1, 2, 0)
    assert rec(stats[1]) == (0, 1, 2, 2, NONE, NONE, NONE, 96_000, 2, 1, 0)
    assert st.stats_lines(stats, [0, 0, 1], ["a", "b", "c"]) == ("0\t2\ta\t96.000\t96.000\ta\tb\t96.000\tb\tc\t1\n"
                                                                 "1\t1\tc\tNA\tNA\tNA\tNA\t96.000\tc\tb\t0\n")
    assert st.not_separated(stats) == 1  # (the member 1 is as close to 2 as to 0)


def test_model_medoid_tie_goes_to_the_smallest_index():
    # 1 and 3 both have the largest row sum; the labelling is not dense and not ordered
    a = matrix(4, {(0, 1): 99.0, (1, 3): 98.0, (3, 2): 99.0, (0, 2): 90.0, (0, 3): 91.0, (1, 2): 91.0})
    cl = [5, 5, 5, 5]
    nodes, stats = st.stats_model(a, cl, 7)
    assert nodes["within_sum"].tolist() == [280_000, 288_000, 280_000, 288_000]
    assert rec(stats[5]) == (1_136_000, 4, 0, 1, 90_000, 0, 2, NONE, NONE, NONE, 0)
    # every pair equal: the medoid is the first member, the minimum's pair (first, second)
    nodes, stats = st.stats_model(matrix(5, {}, fill=97.0), [1, 0, 1, 0, 1], 2)
    assert rec(stats[0]) == (194_000, 2, 1, 1, 97_000, 1, 3, 97_000, 1, 0, 0)
    assert rec(stats[1]) == (582_000, 3, 0, 0, 97_000, 0, 2, 97_000, 0, 1, 0)


def test_model_singleton_and_empty_cluster_id():
    a = matrix(3, {(0, 1): 80.0, (0, 2): 70.0, (1, 2): 99.5})
    nodes, stats = st.stats_model(a, [3, 1, 1], 4)
    assert rec(nodes[0]) == (0, NONE, NONE, 80_000, 1)
    assert rec(stats[3]) == (0, 1, 0, 0, NONE, NONE, NONE, 80_000, 0, 1, 0)  # a singleton is its own medoid
    for empty in (0, 2):
        assert rec(stats[empty]) == (0, 0, NONE, NONE, NONE, NONE, NONE, NONE, NONE, NONE, 0)
    assert rec(stats[1]) == (199_000, 2, 1, 1, 99_500, 1, 2, 80_000, 1, 0, 0)
    text = st.stats_lines(stats[[1, 3]], [0, 1, 1], ["x", "y", "z"])
    assert text.splitlines()[1] == "1\t1\tx\tNA\tNA\tNA\tNA\t80.000\tx\ty\t1"
    # no items at all: n_clusters empty records
    nodes, stats = st.stats_model(np.zeros((0, 0), np.float32), [], 2)
    assert nodes.size == 0 and [rec(x) for x in stats] == [(0, 0, NONE, NONE, NONE, NONE, NONE, NONE, NONE, NONE, 0)] * 2


def test_model_asymmetric_matrix_and_values_outside_the_range():
    a = np.array([[np.nan, 90.0, 50.0],
                  [10.0, -3.0, 60.0],
                  [250.0, np.nan, 1e30]], np.float32)
    nodes, stats = st.stats_model(a, [0, 0, 1], 2)
    # row 0 reads a[0, 1] and a[0, 2] alone; row 1 a[1, 0], a[1, 2]; row 2: 250 counts as 100, NaN as 0; no diagonal
    assert [rec(x) for x in nodes] == [(90_000, 90_000, 1, 50_000, 2), (10_000, 10_000, 0, 60_000, 2), (0, NONE, NONE, 100_000, 0)]
    assert rec(stats[0]) == (100_000, 2, 0, 0, 10_000, 1, 0, 60_000, 1, 2, 0)
    assert rec(stats[1]) == (0, 1, 2, 2, NONE, NONE, NONE, 100_000, 2, 0, 0)
    assert st.not_separated(stats) == 1
    # the transpose is another question with another answer
    assert rec(st.stats_model(a.T.copy(), [0, 0, 1], 2)[1][0]) != rec(stats[0])
