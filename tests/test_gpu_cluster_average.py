"""Average linkage on the device (hg_cluster_average*, `hyper-gen cluster --hclust average`): rep, cluster, into, level (by
its bits), size and the cluster count EQUAL to the models of tests/cluster_average_ref.py -- the matrix form on crafted
matrices (the edges of the mirror tile and of the row scan, two pairs merging in one round, a chain that merges one pair per
round, ties everywhere, the threshold's boundary), with garbage outside the upper triangle, with each optional output
absent, one round per readback and the default; resident sketches against the oracle's matrix under both symmetric
metrics and against hg_dist_full_dev's matrix in blocks of several heights, on a borrowed stream and through the host
form; and end to end through the command line."""
import os
import subprocess
import sys

import numpy as np
import pytest

import cluster_average_ref as av
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
    for key in ("average_rounds", "average_block_rows"):
        c.set_debug(key, "0")
    c.set_ani_metric(cr.MASH)


def run_matrix(gctx, a, th, want=("into", "level", "size")):
    """hg_cluster_average_matrix_dev on the float matrix a -> numpy (rep, cluster, into, level, size, count); an output not in
    `want` is passed as NULL and comes back as None"""
    import torch
    c, hg, dev = gctx
    n = a.shape[0]
    d = torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev) if n else None
    out = {k: torch.full((max(n, 1),), -1, dtype=torch.float32 if k == "level" else torch.int32, device=dev)
           for k in ("rep", "cluster", "into", "level", "size")}
    torch.cuda.synchronize()  # (the ctx runs on its own stream)
    nc = c.cluster_average_matrix_dev(d.data_ptr() if n else None, n, th, out["rep"].data_ptr(), out["cluster"].data_ptr(),
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


def against_model(gctx, a, th, model=av.average_model_rounds):
    """one round per readback and the default: the same result and the same round count, equal to the model's"""
    c = gctx[0]
    want = av.average_model_rounds(a, th, with_rounds=True) if model is av.average_model_rounds else model(a, th) + (None,)
    c.set_debug("average_rounds", "1")
    one = run_matrix(gctx, a, th)
    rounds_one = c.cluster_average_rounds()
    c.set_debug("average_rounds", "0")
    got = run_matrix(gctx, a, th)
    assert c.cluster_average_rounds() == rounds_one  # (the rounds queued behind the last one do not count)
    assert_same(one, want)
    assert_same(got, want)
    if want[6] is not None:
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
    assert c.cluster_average_matrix_dev(None, 0, 95.0, None, None) == 0
    got, rounds = against_model(gctx, np.zeros((1, 1), np.float32), 95.0, av.average_model)
    assert (got[0].tolist(), got[1].tolist(), got[2].tolist(), got[3].tolist(), got[4].tolist(), got[5]) == ([0], [0], [0], [0.0], [1], 1)


@pytest.mark.parametrize("n", [2, 3])
def test_tiny(gctx, n):
    rng = np.random.default_rng(n)
    for th in (0.0, 80.0, 90.0, 99.0):
        a = sym(rng.uniform(75.0, 100.0, (n, n)))
        against_model(gctx, a, th, av.average_model)
    a = matrix(3, {(0, 1): 96.0, (1, 2): 96.0, (0, 2): 0.0})  # single linkage: one cluster; average linkage: two
    got, _ = against_model(gctx, a, 95.0, av.average_model)
    assert got[0].tolist() == [0, 0, 2] and got[5] == 2 and got[3].tolist() == [0.0, 96.0, 0.0]


def test_two_pairs_merge_in_one_round_and_then_with_each_other(gctx):
    a = matrix(4, {(0, 1): 99.0, (2, 3): 98.0, (0, 2): 90.0, (0, 3): 91.0, (1, 2): 92.0, (1, 3): 93.0})
    got, rounds = against_model(gctx, a, 91.5)
    assert_same(got, av.average_model(a, 91.5))
    assert (got[2].tolist(), got[4].tolist(), got[5], rounds) == ([0, 0, 0, 2], [4, 2, 4, 2], 1, 3)
    assert got[3][2] == np.float32(91.5)  # the cross sum of the two passes: (90 + 91 + 92 + 93) / 4
    got, _ = against_model(gctx, a, 91.501)
    assert got[5] == 2
    # an index tie: {1, 2} and {0, 3} equal and best
    a = matrix(4, {(1, 2): 99.0, (0, 3): 99.0}, fill=96.0)
    got, _ = against_model(gctx, a, 95.0)
    assert_same(got, av.average_model(a, 95.0))
    assert got[2].tolist() == [0, 0, 1, 0] and got[4].tolist() == [4, 4, 2, 2]


@pytest.mark.parametrize("n", [65, 257])
def test_random_at_the_edges_of_the_mirror_tile_and_the_row_scan(gctx, n):
    rng = np.random.default_rng(n)
    a = sym(rng.uniform(80.0, 100.0, (n, n)))
    got, rounds = against_model(gctx, a, 90.2)
    assert 1 < got[5] < n
    if n == 65:
        assert_same(got, av.average_model(a, 90.2))
    got, _ = against_model(gctx, a, 0.0)
    assert got[5] == 1 and got[4][0] == n


def test_random_merged_to_one_cluster(gctx):
    rng = np.random.default_rng(300)
    a = sym(rng.uniform(60.0, 100.0, (300, 300)))
    got, rounds = against_model(gctx, a, 0.0)
    assert got[5] == 1 and not got[0].any()
    print("random 300 to one cluster: %d rounds" % rounds)
    assert 10 <= rounds <= 60


def chain(n):
    """neighbours k, k + 1 at 99 - k * 0.05, everything else 0: the strongest pair is always at the front"""
    a = np.zeros((n, n), np.float32)
    k = np.arange(n - 1)
    a[k, k + 1] = a[k + 1, k] = (99.0 - k * 0.05).astype(np.float32)
    return a


def test_chain_whose_similarities_fall_with_the_index(gctx):
    a = chain(64)
    got, rounds = against_model(gctx, a, 0.0)
    assert_same(got, av.average_model(a, 0.0))
    assert got[5] == 1
    print("chain of 64: %d rounds" % rounds)
    assert rounds >= 20  # (far from the log2 n of groups: the accepted worst case)
    got, _ = against_model(gctx, a, 40.0)
    assert 1 < got[5] < 64


def test_ties_everywhere(gctx):
    rng = np.random.default_rng(200)
    a = sym(rng.integers(0, 4, (200, 200)) * 25.0)
    for th in (0.0, 30.0, 50.0, 75.0):
        got, rounds = against_model(gctx, a, th)
    a = sym(rng.integers(0, 4, (60, 60)) * 25.0)
    got, _ = against_model(gctx, a, 40.0)
    assert_same(got, av.average_model(a, 40.0))


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
    assert rounds <= 12


def test_threshold_boundary(gctx):
    th = 95.0  # th_milli = 95 000
    # c(A) c(B) = 1: S == th_milli merges, S - 1 does not (94.9996 prints 95.000 though it is below 95 as a float)
    at, below = np.float32(94.9996), np.nextafter(np.float32(94.9995), np.float32(0))
    assert av.milli(at) == 95_000 and av.milli(below) == 94_999
    assert against_model(gctx, matrix(2, {(0, 1): at}), th, av.average_model)[0][5] == 1
    assert against_model(gctx, matrix(2, {(0, 1): below}), th, av.average_model)[0][5] == 2
    # c(A) c(B) = 6: {0, 1} and {2, 3, 4} form at 99; their six cross pairs sum to 6 * 95 000 exactly, or to one less
    pairs = {(0, 1): 99.0, (2, 3): 99.0, (2, 4): 99.0, (3, 4): 99.0}
    cross = [(i, j) for i in (0, 1) for j in (2, 3, 4)]
    exact = {**pairs, **dict(zip(cross, (95.003, 94.997, 95.001, 94.999, 95.0, 95.0)))}
    assert sum(av.milli(exact[p]) for p in cross) == 6 * 95_000
    got, _ = against_model(gctx, matrix(5, exact), th, av.average_model)
    assert got[5] == 1 and got[4].tolist() == [5, 2, 5, 2, 3] and got[3][2] == np.float32(95.0)
    less = dict(exact)
    less[(1, 4)] = 94.999
    assert sum(av.milli(less[p]) for p in cross) == 6 * 95_000 - 1
    got, _ = against_model(gctx, matrix(5, less), th, av.average_model)
    assert got[5] == 2 and got[0].tolist() == [0, 0, 2, 2, 2]
    # thresholds that merge nothing, and everything
    a = matrix(3, {(0, 1): 100.0, (0, 2): 100.0, (1, 2): 100.0})
    for t, count in ((np.nan, 3), (100.001, 3), (100.0, 1), (0.0, 1), (-5.0, 1)):
        got, rounds = against_model(gctx, a, t, av.average_model)
        assert got[5] == count and (rounds == 0) == (count == 3)


def test_only_the_upper_triangle_is_read(gctx):
    rng = np.random.default_rng(5)
    a = sym(rng.uniform(85.0, 100.0, (130, 130)))
    want = av.average_model_rounds(a, 92.5)
    b = a.copy()
    low = np.tril_indices(130)
    b[low] = rng.uniform(-1e30, 1e30, low[0].size).astype(np.float32)
    b[np.arange(130), np.arange(130)] = np.nan
    b[5, 2], b[7, 7], b[100, 3] = np.inf, -np.inf, np.nan
    assert_same(run_matrix(gctx, b, 92.5), want)
    # values outside [0, 100] inside the triangle count as dist would print them
    a[0, 1] = a[1, 0] = np.nan
    a[2, 9] = a[9, 2] = 250.0
    a[3, 4] = a[4, 3] = -7.0
    against_model(gctx, a, 92.5)


def test_each_optional_output_may_be_absent(gctx):
    a = grouped(np.random.default_rng(9), 6, 7)
    want = av.average_model_rounds(a, 95.0)
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
            c.cluster_average_matrix_dev(*args)
        assert e.value.status == hg.ERR_INVALID


def test_beyond_the_limit_is_unsupported_and_the_next_call_starts_clean(gctx):
    import torch
    c, hg, dev = gctx
    d = torch.zeros(16, dtype=torch.float32, device=dev)  # (never read: the size is refused before anything is allocated)
    out = torch.zeros(4, dtype=torch.int32, device=dev)
    with pytest.raises(hg.HgError) as e:
        c.cluster_average_matrix_dev(d.data_ptr(), hg.CLUSTER_AVERAGE_MAX_N + 1, 95.0, out.data_ptr(), out.data_ptr())
    assert e.value.status == hg.ERR_UNSUPPORTED
    with pytest.raises(hg.HgError) as e:
        c.cluster_average_dev(d.data_ptr(), d.data_ptr(), hg.CLUSTER_AVERAGE_MAX_N + 1, 4096, out.data_ptr(), out.data_ptr())
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
    c.set_ani_metric(metric)
    want = av.average_model_rounds(mats[metric], th)
    assert_same(c.cluster_average(hv, n2, 21, th), want)
    p = np.arange(hv.shape[0])[::-1]
    m = np.ascontiguousarray(mats[metric][np.ix_(p, p)])
    want_rev = av.average_model_rounds(m, th)
    assert_same(c.cluster_average(np.ascontiguousarray(hv[p]), np.ascontiguousarray(n2[p]), 21, th), want_rev)
    assert want[5] == want_rev[5]  # (ties aside the partition does not depend on the order; the count is printed either way)
    print("th %.1f metric %d: %d average-linkage clusters in %d rounds" % (th, metric, want[5], c.cluster_average_rounds()))


def test_directional_metric_is_invalid(gctx, real_sketches):
    c, hg, dev = gctx
    hv, n2, mats = real_sketches
    c.set_ani_metric(cr.CONTAINMENT)
    with pytest.raises(hg.HgError) as e:
        c.cluster_average(hv, n2, 21, 95.0)
    assert e.value.status == hg.ERR_INVALID
    assert "HG_ANI_CONTAINMENT is directional" in str(e.value)


# ---- hg_cluster_average_dev on the bench's clustered HVs --------------------------------------------------------------
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


def average_dev(c, hv, n2, th, n=N_BENCH):
    import torch
    out = {k: torch.full((n,), -1, dtype=torch.float32 if k == "level" else torch.int32, device=hv.device)
           for k in ("rep", "cluster", "into", "level", "size")}
    torch.cuda.synchronize()
    nc = c.cluster_average_dev(hv.data_ptr(), n2.data_ptr(), n, hv.shape[1], out["rep"].data_ptr(), out["cluster"].data_ptr(),
                               out["into"].data_ptr(), out["level"].data_ptr(), out["size"].data_ptr(), 21, th)
    torch.cuda.synchronize()
    h = {k: v.cpu().numpy() for k, v in out.items()}
    return h["rep"].view(np.uint32), h["cluster"].view(np.uint32), h["into"].view(np.uint32), h["level"], h["size"].view(np.uint32), nc


@pytest.mark.parametrize("where", ["95", "median"])
def test_average_dev_clustered(gctx, clustered, where):
    import torch
    c, hg, dev = gctx
    hv, n2, full, median = clustered
    th = 95.0 if where == "95" else median
    want = av.average_model_rounds(full, th, with_rounds=True)
    got = average_dev(c, hv, n2, th)
    assert_same(got, want)
    assert c.cluster_average_rounds() == want[6]
    print("clustered at %s (%.3f): %d clusters in %d rounds" % (where, th, got[5], want[6]))
    # blocks of 7, 64 and all rows of the ANI matrix; a borrowed stream
    for rows in ("7", "64", "1000"):
        c.set_debug("average_block_rows", rows)
        assert_same(average_dev(c, hv, n2, th), want)
    c.set_debug("average_block_rows", "0")
    c.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    try:
        assert_same(average_dev(c, hv, n2, th), want)
    finally:
        c.reset_stream()
    # the host form, on the first 300 rows
    h_hv, h_n2 = hv[:300].cpu().numpy(), n2[:300].cpu().numpy()
    assert_same(c.cluster_average(h_hv, h_n2, 21, th), av.average_model_rounds(full[:300, :300], th))
    if where == "median":
        # the scheme's property, directly on the full matrix: the exact average of milli between any two final clusters is
        # below th_milli (S < th_milli c c'), and the clusters are more than the groups
        assert got[5] > 10
        m = av.milli_matrix(full)
        m = np.triu(m, 1)
        m = m + m.T
        onehot = np.zeros((N_BENCH, got[5]), np.int64)
        onehot[np.arange(N_BENCH), got[1]] = 1
        s = onehot.T @ m @ onehot
        cnt = onehot.sum(0)
        bound = av.th_milli(th) * cnt[:, None] * cnt[None, :]
        off = ~np.eye(got[5], dtype=bool)
        assert (s[off] < bound[off]).all()


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


def test_cli_hclust_average_end_to_end(gctx, tmp_path):
    c, hg, dev = gctx
    from oracle import oracle as orc
    orc.lib()
    d = tmp_path / "fa"
    d.mkdir()
    ids = [40, 35, 0, 3, 199, 101, 140, 100, 300]
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
    for th in ("95", "97.5"):
        rep, cl, into, level, size, nc = av.average_model(ani, float(th))
        out, tree = str(tmp_path / ("avg%s.tsv" % th)), str(tmp_path / ("tree%s.tsv" % th))
        r = cli(hg, "cluster", "-p", sk, "-o", out, "-a", th, "--hclust", "average", "--tree", tree)
        want = "".join("%s\t%d\t%s\n" % (files[i], cl[i], files[rep[i]]) for i in range(n)).encode()
        assert open(out, "rb").read() == want
        want_tree = "".join("%s\t%s\t%.3f\t%d\n" % (files[into[b]], files[b], float(level[b]), size[b])
                            for b in av.merge_order(into, level, size)).encode()
        got_tree = open(tree, "rb").read()
        assert got_tree == want_tree and got_tree.count(b"\n") == n - nc
        singletons = int((np.bincount(cl) == 1).sum())
        assert ("Output %d genomes in %d clusters (%d singletons) at ANI threshold %.1f to file %s" % (n, nc, singletons, float(th), out)) in r.stdout
        assert "Clustered %d files took" % n in r.stdout
        # without --tree: the same clusters
        out2 = str(tmp_path / ("avg%s_notree.tsv" % th))
        cli(hg, "cluster", "-p", sk, "-o", out2, "-a", th, "--hclust=average")
        assert open(out2, "rb").read() == want
    assert 1 < av.average_model(ani, 95.0)[5] < n
