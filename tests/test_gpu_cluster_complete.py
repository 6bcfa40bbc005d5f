"""Complete linkage on the device (hg_cluster_complete*, `hyper-gen cluster --agglomerate complete`): rep, cluster, into,
level (by its bits), size and the cluster count EQUAL to the round model of tests/cluster_complete_ref.py -- the matrix form
on crafted matrices (the edges of the mirror tile, of the row scan's step and of the row padding, two pairs merging in one
round, a chain that merges one pair per round, ties everywhere, the threshold's boundary), with garbage outside the upper
triangle, with each optional output absent, one round per readback against the default and every row scanned every round
against the default; resident sketches against the oracle's matrix under both symmetric metrics and against
hg_dist_full_dev's matrix in blocks of several heights, on a borrowed stream and through the host form; the scheme's
property through hg_cluster_stats_matrix_dev; and end to end through the command line."""
import os
import subprocess
import sys

import numpy as np
import pytest

import cluster_complete_ref as cp
import cluster_stats_ref as st
import containment_ref as cr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gctx():
    import torch
    import hypergen_amd as hg
    with hg.Context(0) as c:
        yield c, hg, torch.device("cuda:0")


@pytest.fixture(autouse=True)
def clean_hooks(gctx):
    yield
    c = gctx[0]
    for key in ("complete_rounds", "complete_block_rows"):
        c.set_debug(key, "0")
    c.set_debug("complete_rescan", "")
    c.set_ani_metric(cr.MASH)


def run_matrix(gctx, a, th, want=("into", "level", "size")):
    """hg_cluster_complete_matrix_dev on the float matrix a -> numpy (rep, cluster, into, level, size, count); an output not
    in `want` is passed as NULL and comes back as None"""
    import torch
    c, hg, dev = gctx
    n = a.shape[0]
    d = torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev) if n else None
    out = {k: torch.full((max(n, 1),), -1, dtype=torch.float32 if k == "level" else torch.int32, device=dev)
           for k in ("rep", "cluster", "into", "level", "size")}
    torch.cuda.synchronize()  # (the ctx runs on its own stream)
    nc = c.cluster_complete_matrix_dev(d.data_ptr() if n else None, n, th, out["rep"].data_ptr(), out["cluster"].data_ptr(),
                                       *(out[k].data_ptr() if k in want else None for k in ("into", "level", "size")))
    host = {k: v[:n].cpu().numpy() for k, v in out.items()}
    return (host["rep"].view(np.uint32), host["cluster"].view(np.uint32), host["into"].view(np.uint32) if "into" in want else None,
            host["level"] if "level" in want else None, host["size"].view(np.uint32) if "size" in want else None, nc)


def assert_same(got, want):
    assert got[5] == want[5], "cluster count"
    for k, name in enumerate(("rep", "cluster", "into", "level", "size")):
        if got[k] is not None:
            assert got[k].dtype == want[k].dtype, name
            assert np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32)), name


def against_model(gctx, a, th):
    """one round per readback, every row scanned every round, and the default: identical arrays and equal round counts,
    equal to the round model's"""
    c = gctx[0]
    want = cp.complete_model_rounds(a, th, with_rounds=True)
    c.set_debug("complete_rounds", "1")
    one = run_matrix(gctx, a, th)
    rounds_one = c.cluster_complete_rounds()
    c.set_debug("complete_rounds", "0")
    c.set_debug("complete_rescan", "all")
    full = run_matrix(gctx, a, th)
    rounds_full = c.cluster_complete_rounds()
    c.set_debug("complete_rescan", "")
    got = run_matrix(gctx, a, th)
    assert c.cluster_complete_rounds() == rounds_one == rounds_full  # (the rounds queued behind the last one do not count)
    assert_same(one, want)
    assert_same(full, want)
    assert_same(got, want)
    assert rounds_one == want[6]
    return got, rounds_one


def sym(a):
    a = np.triu(np.asarray(a, np.float32), 1)
    return a + a.T


def matrix(n, pairs, fill=0.0):
    a = np.full((n, n), fill, np.float32)
    for (i, j), v in pairs.items():
        a[i, j] = a[j, i] = v
    return a


# ---- crafted matrices -----------------------------------------------------------------------------------------------
def test_empty_and_single(gctx):
    c, hg, dev = gctx
    assert c.cluster_complete_matrix_dev(None, 0, 95.0, None, None) == 0
    got, rounds = against_model(gctx, np.zeros((1, 1), np.float32), 95.0)
    assert (got[0].tolist(), got[1].tolist(), got[2].tolist(), got[3].tolist(), got[4].tolist(), got[5]) == ([0], [0], [0], [0.0], [1], 1)


@pytest.mark.parametrize("n", [2, 3])
def test_tiny(gctx, n):
    rng = np.random.default_rng(n)
    for th in (0.0, 80.0, 90.0, 99.0):
        a = sym(rng.uniform(75.0, 100.0, (n, n)))
        got, _ = against_model(gctx, a, th)
        assert_same(got, cp.complete_model(a, th))
    a = matrix(3, {(0, 1): 96.0, (1, 2): 96.0, (0, 2): 0.0})  # single linkage: one cluster; complete linkage: two
    got, _ = against_model(gctx, a, 95.0)
    assert got[0].tolist() == [0, 0, 2] and got[5] == 2 and got[3].tolist() == [0.0, 96.0, 0.0]
    assert against_model(gctx, a, 0.001)[0][5] == 2  # the third joins only at threshold 0
    got, _ = against_model(gctx, a, 0.0)
    assert got[2].tolist() == [0, 0, 0] and got[3].tolist() == [0.0, 96.0, 0.0] and got[4].tolist() == [3, 2, 3]


def test_two_pairs_merge_in_one_round_and_get_the_minimum_of_four(gctx):
    for low in ((0, 2), (0, 3), (1, 2), (1, 3)):  # the minimum in each of the four places the two passes fold
        a = matrix(4, {(0, 1): 99.0, (2, 3): 98.0, (0, 2): 93.0, (0, 3): 93.0, (1, 2): 93.0, (1, 3): 93.0, low: 90.5})
        got, rounds = against_model(gctx, a, 90.5)
        assert_same(got, cp.complete_model(a, 90.5))
        assert (got[2].tolist(), got[4].tolist(), got[5], rounds) == ([0, 0, 0, 2], [4, 2, 4, 2], 1, 3)
        assert got[3].tolist() == [0.0, 99.0, 90.5, 98.0]
        assert against_model(gctx, a, 90.501)[0][5] == 2
    # all six pairs equal: index ties decide every merge
    got, _ = against_model(gctx, matrix(4, {}, fill=97.0), 95.0)
    assert got[2].tolist() == [0, 0, 0, 0] and got[4].tolist() == [4, 2, 3, 4]


@pytest.mark.parametrize("n", [33, 65])
def test_random_at_the_edges_of_the_mirror_tile(gctx, n):
    rng = np.random.default_rng(n)
    a = sym(rng.uniform(80.0, 100.0, (n, n)))
    got, rounds = against_model(gctx, a, 86.0)
    assert 1 < got[5] < n
    assert_same(got, cp.complete_model(a, 86.0))
    got, _ = against_model(gctx, a, 0.0)
    assert got[5] == 1 and got[4][0] == n


@pytest.mark.parametrize("n", [1023, 1025, 1027, 2051, 3077])
def test_row_scan_step_and_row_padding(gctx, n):
    """one step of the row scan covers 1024 columns, a trip of its loop two steps, a single step may follow: one step less
    one column, one step plus 1 and plus 3, one trip plus 3, one trip, a second trip of a few lanes and a step.  Rows are
    padded by 1, 3, 1, 1 and 3 entries.  Groups whose best partners sit anywhere in a row, and one strong pair in the last two
    columns"""
    rng = np.random.default_rng(n)
    a = rng.uniform(60.0, 80.0, (n, n))
    g = rng.permutation(n) % 150  # 150 groups, members scattered over the whole row
    within = g[:, None] == g[None, :]
    a[within] = rng.uniform(96.0, 99.0, int(within.sum()))
    a = sym(a)
    a[n - 2, n - 1] = a[n - 1, n - 2] = 99.999
    a[0, n - 1] = a[n - 1, 0] = 99.998
    got, rounds = against_model(gctx, a, 95.0)
    assert got[0][n - 1] == got[0][n - 2]  # the best pair of all sits in the last two columns, and merges
    assert 1 < got[5] < n
    print("n %d: %d clusters in %d rounds" % (n, got[5], rounds))


def test_random_merged_to_one_cluster(gctx):
    rng = np.random.default_rng(300)
    a = sym(rng.uniform(60.0, 100.0, (300, 300)))
    got, rounds = against_model(gctx, a, 0.0)
    assert got[5] == 1 and not got[0].any()
    print("random 300 to one cluster: %d rounds" % rounds)


def chain(n):
    """neighbours k, k + 1 at 99 - k * 0.05, everything else 0: the strongest pair is always at the front"""
    a = np.zeros((n, n), np.float32)
    k = np.arange(n - 1)
    a[k, k + 1] = a[k + 1, k] = (99.0 - k * 0.05).astype(np.float32)
    return a


def test_chain_whose_similarities_fall_with_the_index(gctx):
    a = chain(64)
    got, rounds = against_model(gctx, a, 0.0)  # (against_model: the round count equals the model's)
    assert_same(got, cp.complete_model(a, 0.0))
    assert got[5] == 1
    print("chain of 64: %d rounds" % rounds)
    assert rounds >= 33  # (the neighbours pair up front to back, one pair per round; the pairs, all at 0, join meanwhile)
    got, rounds = against_model(gctx, a, 40.0)
    assert got[5] == 32 and rounds == 33  # one merge per round, 32 of them, and the round that merges nothing


def test_ties_everywhere(gctx):
    rng = np.random.default_rng(200)
    a = sym(rng.integers(0, 4, (200, 200)) * 25.0)
    for th in (0.0, 30.0, 50.0, 75.0):
        got, rounds = against_model(gctx, a, th)
    a = sym(rng.integers(0, 4, (60, 60)) * 25.0)
    got, _ = against_model(gctx, a, 40.0)
    assert_same(got, cp.complete_model(a, 40.0))


def grouped(rng, groups, size):
    n = groups * size
    a = rng.uniform(80.0, 90.0, (n, n))
    g = np.arange(n) // size
    within = g[:, None] == g[None, :]
    a[within] = rng.uniform(97.0, 99.9, int(within.sum()))
    return sym(a)


def test_groups(gctx):
    a = grouped(np.random.default_rng(400), 40, 10)
    got, rounds = against_model(gctx, a, 95.0)
    assert got[5] == 40 and np.array_equal(got[0], (np.arange(400) // 10 * 10).astype(np.uint32))
    print("40 groups of 10: %d rounds" % rounds)
    got, _ = against_model(gctx, a, 98.5)  # inside the groups' band: the groups fall apart into cliques at 98.5
    assert got[5] > 40


def test_threshold_boundary(gctx):
    th = 95.0  # th_milli = 95 000
    at, below = np.float32(94.9996), np.nextafter(np.float32(94.9995), np.float32(0))
    assert cp.milli(at) == 95_000 and cp.milli(below) == 94_999
    assert against_model(gctx, matrix(2, {(0, 1): at}), th)[0][5] == 1
    assert against_model(gctx, matrix(2, {(0, 1): below}), th)[0][5] == 2
    # {0, 1} and {2, 3, 4} form at 99; the lowest of their six cross pairs is th_milli exactly, or one less
    pairs = {(0, 1): 99.0, (2, 3): 99.0, (2, 4): 99.0, (3, 4): 99.0}
    cross = [(i, j) for i in (0, 1) for j in (2, 3, 4)]
    exact = {**pairs, **dict(zip(cross, (95.003, 96.0, 95.001, 95.0, 97.0, 95.002)))}
    got, _ = against_model(gctx, matrix(5, exact), th)
    assert got[5] == 1 and got[4].tolist() == [5, 2, 5, 2, 3] and got[3][2] == np.float32(95.0)
    less = dict(exact)
    less[(1, 2)] = 94.999
    got, _ = against_model(gctx, matrix(5, less), th)
    assert got[5] == 2 and got[0].tolist() == [0, 0, 2, 2, 2]
    # thresholds that merge nothing, and everything (pairs of ANI 0 and NaN included)
    a = matrix(3, {(0, 1): 100.0, (0, 2): 100.0, (1, 2): 100.0})
    for t, count in ((np.nan, 3), (100.001, 3), (100.0, 1), (0.0, 1), (-5.0, 1)):
        got, rounds = against_model(gctx, a, t)
        assert got[5] == count and (rounds == 0) == (count == 3)
    a = matrix(4, {(0, 1): np.nan, (2, 3): 50.0})
    for t in (0.0, -1.0):
        got, _ = against_model(gctx, a, t)
        assert got[5] == 1 and got[2].tolist() == [0, 0, 0, 2] and got[3].tolist() == [0.0, 0.0, 0.0, 50.0]


def test_only_the_upper_triangle_is_read(gctx):
    rng = np.random.default_rng(5)
    a = sym(rng.uniform(85.0, 100.0, (130, 130)))
    want = cp.complete_model_rounds(a, 88.5)
    assert 1 < want[5] < 130
    b = a.copy()
    b[np.tril_indices(130)] = np.nan  # a NaN lower triangle and diagonal are never read
    assert_same(run_matrix(gctx, b, 88.5), want)
    low = np.tril_indices(130)
    b[low] = rng.uniform(-1e30, 1e30, low[0].size).astype(np.float32)
    b[5, 2], b[7, 7], b[100, 3] = np.inf, -np.inf, np.nan
    assert_same(run_matrix(gctx, b, 88.5), want)
    # values outside [0, 100] inside the triangle count as dist would print them
    a[0, 1] = a[1, 0] = np.nan
    a[2, 9] = a[9, 2] = 250.0
    a[3, 4] = a[4, 3] = -7.0
    against_model(gctx, a, 88.5)


def test_each_optional_output_may_be_absent(gctx):
    a = grouped(np.random.default_rng(9), 6, 7)
    want = cp.complete_model_rounds(a, 95.0)
    for absent in ("into", "level", "size"):
        keep = tuple(k for k in ("into", "level", "size") if k != absent)
        got = run_matrix(gctx, a, 95.0, want=keep)
        assert got[("into", "level", "size").index(absent) + 2] is None
        assert_same(got, want)
    assert_same(run_matrix(gctx, a, 95.0, want=()), want)


def test_null_arguments_are_invalid(gctx):
    import torch
    c, hg, dev = gctx
    d = torch.zeros(9, dtype=torch.float32, device=dev)
    out = torch.zeros(3, dtype=torch.int32, device=dev)
    for args in ((None, 3, 95.0, out.data_ptr(), out.data_ptr()), (d.data_ptr(), 3, 95.0, None, out.data_ptr()),
                 (d.data_ptr(), 3, 95.0, out.data_ptr(), None)):
        with pytest.raises(hg.HgError) as e:
            c.cluster_complete_matrix_dev(*args)
        assert e.value.status == hg.ERR_INVALID


def test_beyond_the_limit_is_unsupported_and_the_next_call_starts_clean(gctx):
    import torch
    c, hg, dev = gctx
    d = torch.zeros(16, dtype=torch.float32, device=dev)  # (never read: the size is refused before anything is allocated)
    out = torch.zeros(4, dtype=torch.int32, device=dev)
    with pytest.raises(hg.HgError) as e:
        c.cluster_complete_matrix_dev(d.data_ptr(), hg.CLUSTER_COMPLETE_MAX_N + 1, 95.0, out.data_ptr(), out.data_ptr())
    assert e.value.status == hg.ERR_UNSUPPORTED
    with pytest.raises(hg.HgError) as e:
        c.cluster_complete_dev(d.data_ptr(), d.data_ptr(), hg.CLUSTER_COMPLETE_MAX_N + 1, 4096, out.data_ptr(), out.data_ptr())
    assert e.value.status == hg.ERR_UNSUPPORTED
    a = matrix(4, {(0, 1): 99.0, (2, 3): 98.0}, fill=50.0)
    against_model(gctx, a, 95.0)


# ---- real sketches against the oracle ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def real_sketches(gctx):
    c, hg, dev = gctx
    from oracle import oracle as orc
    orc.lib()
    # four roots, members at 0 .. 9.8 % substitutions (synth_genome: member m of a cluster carries m * 0.1 %)
    ids = [r * 100 + m for r in range(4) for m in range(0, 100, 2)]
    seqs = [orc.synth_genome(g, 60_000) for g in ids]
    hv, n2, nh = c.sketch_batch(seqs, hg.default_params(scaled=60))
    mats = {cr.MASH: orc.ani_matrix(hv, n2, hv, n2, 21),
            cr.MAX_CONTAINMENT: cr.ani_ref(orc, cr.exact_dots(hv, hv), n2[:, None], n2[None, :], 21, cr.MAX_CONTAINMENT)}
    return hv, n2, mats


@pytest.mark.parametrize("metric", [cr.MASH, cr.MAX_CONTAINMENT])
@pytest.mark.parametrize("th", [85.0, 95.0, 99.0, 99.9])
def test_real_sketches_against_oracle(gctx, real_sketches, th, metric):
    """the host form in file order and reversed, against the model on the oracle's matrix"""
    c, hg, dev = gctx
    hv, n2, mats = real_sketches
    assert hv.shape[0] == 200
    c.set_ani_metric(metric)
    want = cp.complete_model_rounds(mats[metric], th)
    assert_same(c.cluster_complete(hv, n2, 21, th), want)
    p = np.arange(hv.shape[0])[::-1]
    m = np.ascontiguousarray(mats[metric][np.ix_(p, p)])
    want_rev = cp.complete_model_rounds(m, th)
    assert_same(c.cluster_complete(np.ascontiguousarray(hv[p]), np.ascontiguousarray(n2[p]), 21, th), want_rev)
    print("th %.1f metric %d: %d complete-linkage clusters (%d reversed) in %d rounds"
          % (th, metric, want[5], want_rev[5], c.cluster_complete_rounds()))


def test_directional_metric_is_invalid(gctx, real_sketches):
    c, hg, dev = gctx
    hv, n2, mats = real_sketches
    c.set_ani_metric(cr.CONTAINMENT)
    with pytest.raises(hg.HgError) as e:
        c.cluster_complete(hv, n2, 21, 95.0)
    assert e.value.status == hg.ERR_INVALID
    assert "HG_ANI_CONTAINMENT is directional" in str(e.value)


# ---- hg_cluster_complete_dev on the bench's clustered HVs -------------------------------------------------------------
N_BENCH = 1_000


@pytest.fixture(scope="module")
def clustered(gctx):
    """(hv, n2, hg_dist_full_dev's matrix on the host, median within-cluster ANI of rows 0..299)"""
    import torch
    c, hg, dev = gctx
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import bench
    hv = bench.clustered_hvs(N_BENCH, 0, dev)
    n2 = (hv.int() ** 2).sum(1).int()
    full = torch.empty(N_BENCH * N_BENCH, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    c.dist_full_dev(hv.data_ptr(), n2.data_ptr(), N_BENCH, hv.data_ptr(), n2.data_ptr(), N_BENCH, hv.shape[1], 21, full.data_ptr())
    c.sync()
    full = full.cpu().numpy().reshape(N_BENCH, N_BENCH)
    i, j = np.triu_indices(300, 1)
    within = full[i, j][i // 100 == j // 100]  # (clustered_hvs: groups of 100 consecutive rows)
    return hv, n2, full, float(np.median(within))


def complete_dev(c, hv, n2, th, n=N_BENCH):
    import torch
    out = {k: torch.full((n,), -1, dtype=torch.float32 if k == "level" else torch.int32, device=hv.device)
           for k in ("rep", "cluster", "into", "level", "size")}
    torch.cuda.synchronize()
    nc = c.cluster_complete_dev(hv.data_ptr(), n2.data_ptr(), n, hv.shape[1], out["rep"].data_ptr(), out["cluster"].data_ptr(),
                                out["into"].data_ptr(), out["level"].data_ptr(), out["size"].data_ptr(), 21, th)
    torch.cuda.synchronize()
    h = {k: v.cpu().numpy() for k, v in out.items()}
    return h["rep"].view(np.uint32), h["cluster"].view(np.uint32), h["into"].view(np.uint32), h["level"], h["size"].view(np.uint32), nc


@pytest.mark.parametrize("where", ["95", "median"])
def test_complete_dev_clustered(gctx, clustered, where):
    import torch
    c, hg, dev = gctx
    hv, n2, full, median = clustered
    th = 95.0 if where == "95" else median
    want = cp.complete_model_rounds(full, th, with_rounds=True)
    got = complete_dev(c, hv, n2, th)
    assert_same(got, want)
    assert c.cluster_complete_rounds() == want[6]
    print("clustered at %s (%.3f): %d clusters in %d rounds" % (where, th, got[5], want[6]))
    c.set_debug("complete_rescan", "all")
    assert_same(complete_dev(c, hv, n2, th), want)
    assert c.cluster_complete_rounds() == want[6]
    c.set_debug("complete_rescan", "")
    # blocks of 7, 64 and all rows of the ANI matrix; a borrowed stream
    for rows in ("7", "64", "1000"):
        c.set_debug("complete_block_rows", rows)
        assert_same(complete_dev(c, hv, n2, th), want)
    c.set_debug("complete_block_rows", "0")
    c.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    try:
        assert_same(complete_dev(c, hv, n2, th), want)
    finally:
        c.reset_stream()
    # the host form, on the first 300 rows
    h_hv, h_n2 = hv[:300].cpu().numpy(), n2[:300].cpu().numpy()
    assert_same(c.cluster_complete(h_hv, h_n2, 21, th), cp.complete_model_rounds(full[:300, :300], th))
    # the scheme's property, through the product's own statistics on the same (symmetric) matrix: the lowest ANI within every
    # cluster of two or more is at least th_milli ...
    t = cp.th_milli(th)
    m = np.triu(full, 1)
    m = m + m.T
    d = torch.from_numpy(np.ascontiguousarray(m, np.float32)).to(dev)
    d_cl = torch.from_numpy(got[1].view(np.int32).copy()).to(dev)
    d_stat = torch.zeros(got[5] * 48, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    c.cluster_stats_matrix_dev(d.data_ptr(), N_BENCH, d_cl.data_ptr(), got[5], None, d_stat.data_ptr())
    stat = d_stat.cpu().numpy().view(st.CLUSTER_DTYPE)
    assert stat["size"].sum() == N_BENCH
    several = stat["size"] >= 2
    assert several.any() and (stat["within_min"][several] >= t).all()
    # ... and, on the host, every two final clusters have a member pair below th_milli (they could not have merged)
    mm = cp.milli_matrix(m)
    onehot = np.zeros((N_BENCH, got[5]), bool)
    onehot[np.arange(N_BENCH), got[1]] = True
    lowest = np.full((got[5], got[5]), 1 << 30, np.int64)
    for x in range(got[5]):
        rows = mm[onehot[:, x]].min(axis=0)  # per item: its lowest m with a member of cluster x
        np.minimum.at(lowest[x], got[1], rows)
    off = ~np.eye(got[5], dtype=bool)
    assert (lowest[off] < t).all()
    if where == "95":
        # the groups are complete cliques at 95: complete linkage and single linkage agree
        rep = torch.empty(N_BENCH, dtype=torch.int32, device=dev)
        cl = torch.empty(N_BENCH, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        nc = c.cluster_dev(hv.data_ptr(), n2.data_ptr(), N_BENCH, hv.shape[1], rep.data_ptr(), cl.data_ptr(), 21, th)
        c.sync()
        assert nc == got[5] == N_BENCH // 100
        assert np.array_equal(rep.cpu().numpy().view(np.uint32), got[0]) and np.array_equal(cl.cpu().numpy().view(np.uint32), got[1])
    else:
        assert got[5] > N_BENCH // 100  # at the median half of a group's pairs are below the threshold


# ---- command line ------------------------------------------------------------------------------------------------------
def write_fasta(path, seq, name):
    s = bytes(seq).decode()
    with open(path, "w") as f:
        f.write(">%s\n" % name)
        for i in range(0, len(s), 80):
            f.write(s[i:i + 80] + "\n")


def cli(hg, *args):
    r = subprocess.run([hg.CLI_PATH] + list(args), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return r


def milli_text(m):
    return "%d.%03d" % (m // 1000, m % 1000)


def test_cli_agglomerate_end_to_end(gctx, tmp_path):
    c, hg, dev = gctx
    from oracle import oracle as orc
    orc.lib()
    d = tmp_path / "fa"
    d.mkdir()
    ids = [40, 35, 0, 3, 199, 101, 140, 100, 300, 20, 120, 310]
    for k, g in enumerate(ids):
        write_fasta(str(d / ("f%02d_g%03d.fna" % (k, g))), orc.synth_genome(g, 200_000)[1:], "g%d" % g)
    sk = str(tmp_path / "all.sketch")
    cli(hg, "sketch", "-p", str(d), "-o", sk, "-s", "100", "-t", "4")
    recs = hg.read_sketch_file(sk)
    files = [x["file_str"] for x in recs]
    n = len(files)
    # model: oracle sketches of the same files, the oracle's ANI matrix
    hvs, n2s = [], []
    for f in files:
        hv, n2, _ = orc.sketch_genome(hg.read_merge_seq(f), ksize=21, scaled=100, norm=orc.NORM_U2T)
        hvs.append(hv), n2s.append(n2)
    hvs, n2s = np.stack(hvs), np.array(n2s, np.int32)
    ani = orc.ani_matrix(hvs, n2s, hvs, n2s, 21)
    mm = cp.milli_matrix(ani)
    for th in ("95", "97.5"):
        rep, cl, into, level, size, nc = cp.complete_model(ani, float(th))
        out, tree, stats = (str(tmp_path / ("%s%s.tsv" % (k, th))) for k in ("cpl", "tree", "stats"))
        r = cli(hg, "cluster", "-p", sk, "-o", out, "-a", th, "--agglomerate", "complete", "--tree", tree, "--stats", stats)
        want = "".join("%s\t%d\t%s\n" % (files[i], cl[i], files[rep[i]]) for i in range(n)).encode()
        assert open(out, "rb").read() == want
        want_tree = "".join("%s\t%s\t%.3f\t%d\n" % (files[into[b]], files[b], float(level[b]), size[b])
                            for b in cp.merge_order(into, level, size)).encode()
        got_tree = open(tree, "rb").read()
        assert got_tree == want_tree and got_tree.count(b"\n") == n - nc
        # --stats: one line per cluster; the lowest ANI within (field 5) is the model's, and at least -a
        lines = [x.split("\t") for x in open(stats).read().splitlines()]
        assert len(lines) == nc
        for k, f in enumerate(lines):
            mem = np.flatnonzero(cl == k)
            assert (int(f[0]), int(f[1])) == (k, mem.size)
            if mem.size >= 2:
                low = min(int(mm[i, j]) for i in mem for j in mem if i < j)
                assert f[4] == milli_text(low) and low >= cp.th_milli(float(th))
            else:
                assert f[4] == "NA"
        singletons = int((np.bincount(cl) == 1).sum())
        assert ("Output %d genomes in %d clusters (%d singletons) at ANI threshold %.1f to file %s" % (n, nc, singletons, float(th), out)) in r.stdout
        # without --tree: the same clusters
        out2 = str(tmp_path / ("cpl%s_notree.tsv" % th))
        cli(hg, "cluster", "-p", sk, "-o", out2, "-a", th, "--agglomerate=complete")
        assert open(out2, "rb").read() == want
        # --agglomerate average writes the bytes of --hclust average
        pair = {}
        for how in ("--agglomerate", "--hclust"):
            o, t, s = (str(tmp_path / ("%s_%s%s.tsv" % (how[2:], k, th))) for k in ("o", "t", "s"))
            cli(hg, "cluster", "-p", sk, "-o", o, "-a", th, how, "average", "--tree", t, "--stats", s)
            pair[how] = tuple(open(x, "rb").read() for x in (o, t, s))
            assert all(pair[how])
        assert pair["--agglomerate"] == pair["--hclust"]
    assert 1 < cp.complete_model(ani, 95.0)[5] < n
