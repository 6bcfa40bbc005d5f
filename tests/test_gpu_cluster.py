"""Single-linkage clustering on the device (hg_cluster*, `hyper-gen cluster`): rep, cluster and the cluster count against
a union-find written here in numpy / Python, equal bit for bit -- on constructed edge lists (worst-case depths, stars,
duplicates, thresholds at the float boundary, split and reordered deliveries), on real sketches against the oracle's ANI
matrix, on the bench's clustered HVs against the hits of hg_dist_dev (row blocks, the grow path, a borrowed stream,
more than 2^32 pairs) and end to end through the command line."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def model(n, a, b):
    """rep / cluster / count of the graph with edges (a[k], b[k]): union-find hooking the larger root under the smaller"""
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for u, v in zip(np.asarray(a).tolist(), np.asarray(b).tolist()):
        ru, rv = find(u), find(v)
        if ru < rv:
            parent[rv] = ru
        elif rv < ru:
            parent[ru] = rv
    rep = np.array([find(x) for x in range(n)], np.uint32)
    roots = np.unique(rep)
    return rep, np.searchsorted(roots, rep).astype(np.uint32), int(roots.size)


def hits_array(a, b, ani):
    import hypergen_amd as hg
    h = np.zeros(len(a), hg.ANI_HIT_DTYPE)
    h["ref_idx"], h["qry_idx"], h["ani"] = a, b, ani
    return h


@pytest.fixture(scope="module")
def gctx():
    import torch
    import hypergen_amd as hg
    with hg.Context(0) as c:
        yield c, hg, torch.device("cuda:0")


def run_hits(gctx, n, batches, th):
    """init, one add_hits call per hit array of `batches`, finish -> numpy rep, cluster, count"""
    import torch
    c, hg, dev = gctx
    rep = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    cl = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    d_batches = [torch.from_numpy(h.view(np.uint8).copy()).to(dev) for h in batches]
    torch.cuda.synchronize()  # (the ctx runs on its own stream)
    c.cluster_init_dev(rep.data_ptr(), n)
    for h, d in zip(batches, d_batches):
        c.cluster_add_hits_dev(rep.data_ptr(), n, d.data_ptr(), h.size, th)
    nc = c.cluster_finish_dev(rep.data_ptr(), n, cl.data_ptr())
    return rep[:n].cpu().numpy().view(np.uint32), cl[:n].cpu().numpy().view(np.uint32), nc


def assert_same(got, want):
    assert got[2] == want[2], "cluster count"
    assert np.array_equal(got[0], want[0]), "rep"
    assert np.array_equal(got[1], want[1]), "cluster"


# ---- constructed edge lists -------------------------------------------------------------------------------------------
def test_random_sparse_graph(gctx):
    rng = np.random.default_rng(11)
    n, m = 200_000, 1_000_000
    a = rng.integers(0, n, m, dtype=np.uint32)
    b = rng.integers(0, n, m, dtype=np.uint32)
    b[:20_000] = a[:20_000]  # self-pairs
    a[20_000:40_000], b[20_000:40_000] = b[40_000:60_000], a[40_000:60_000]  # both orientations of the same pairs
    a[60_000:80_000], b[60_000:80_000] = a[80_000:100_000], b[80_000:100_000]  # duplicates
    ani = rng.uniform(80.0, 100.0, m).astype(np.float32)
    keep = ani >= np.float32(95.0)
    want = model(n, a[keep], b[keep])
    got = run_hits(gctx, n, [hits_array(a, b, ani)], 95.0)
    assert_same(got, want)
    assert 1 < got[2] < n


@pytest.mark.parametrize("order", ["shuffled", "descending"])
def test_path_of_a_million(gctx, order):
    n = 1_000_000
    rng = np.random.default_rng(5)
    if order == "shuffled":  # a path through the nodes in random order, its edges delivered in random order
        perm = rng.permutation(n).astype(np.uint32)
        e = rng.permutation(n - 1)
        a, b = perm[e], perm[e + 1]
    else:
        k = np.arange(n - 2, -1, -1, dtype=np.uint32)
        a, b = k + 1, k
    got = run_hits(gctx, n, [hits_array(a, b, 100.0)], 95.0)
    assert got[2] == 1
    assert not got[0].any() and not got[1].any()


def test_star_on_the_last_index(gctx):
    n = 300_000
    k = np.arange(n - 1, dtype=np.uint32)
    a = np.full(n - 1, n - 1, np.uint32)
    got = run_hits(gctx, n, [hits_array(a[::2], k[::2], 99.0)], 95.0)
    assert_same(got, model(n, a[::2], k[::2]))
    assert got[2] == n - (n - 1 + 1) // 2


def test_empty_and_single(gctx):
    got = run_hits(gctx, 1000, [], 95.0)
    assert_same(got, (np.arange(1000, dtype=np.uint32), np.arange(1000, dtype=np.uint32), 1000))
    got = run_hits(gctx, 1000, [hits_array([], [], [])], 95.0)
    assert got[2] == 1000
    got = run_hits(gctx, 1, [hits_array([0], [0], [100.0])], 95.0)
    assert_same(got, (np.zeros(1, np.uint32), np.zeros(1, np.uint32), 1))


def test_threshold_boundary(gctx):
    th = np.float32(95.0)
    below = np.nextafter(th, np.float32(0))
    a = np.array([0, 2, 4, 6], np.uint32)
    b = np.array([1, 3, 5, 7], np.uint32)
    ani = np.array([th, below, th, below], np.float32)
    got = run_hits(gctx, 8, [hits_array(a, b, ani)], float(th))
    assert_same(got, model(8, [0, 4], [1, 5]))
    assert list(got[0]) == [0, 0, 2, 3, 4, 4, 6, 7] and got[2] == 6
    # one hit list clustered at several thresholds without another comparison
    assert run_hits(gctx, 8, [hits_array(a, b, ani)], float(below))[2] == 4


def test_split_and_reordered_delivery_is_identical(gctx):
    rng = np.random.default_rng(23)
    n, m = 50_000, 120_000
    a = rng.integers(0, n, m, dtype=np.uint32)
    b = rng.integers(0, n, m, dtype=np.uint32)
    h = hits_array(a, b, 97.0)
    want = model(n, a, b)
    one = run_hits(gctx, n, [h], 95.0)
    assert_same(one, want)
    p = rng.permutation(m)
    parts = [h[p[i:i + 7_001]] for i in range(0, m, 7_001)]
    assert_same(run_hits(gctx, n, parts, 95.0), want)
    assert_same(run_hits(gctx, n, [h[::-1].copy()], 95.0), want)


def test_index_out_of_range_is_invalid(gctx):
    c, hg, dev = gctx
    with pytest.raises(hg.HgError) as e:
        run_hits(gctx, 100, [hits_array([1, 3], [2, 100], [99.0, 99.0])], 95.0)
    assert e.value.status == hg.ERR_INVALID
    # the next clustering on the ctx starts clean; a bad index below the threshold is an error too
    assert run_hits(gctx, 100, [hits_array([1], [2], [99.0])], 95.0)[2] == 99
    with pytest.raises(hg.HgError):
        run_hits(gctx, 100, [hits_array([1], [5000], [10.0])], 95.0)


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
    return orc, hv, n2


@pytest.mark.parametrize("th", [85.0, 95.0, 99.0, 99.9])
def test_real_sketches_against_oracle(gctx, real_sketches, th):
    c, hg, dev = gctx
    orc, hv, n2 = real_sketches
    n = hv.shape[0]
    ani = orc.ani_matrix(hv, n2, hv, n2, 21)
    i, j = np.nonzero(np.triu(ani >= np.float32(th), 1))
    want = model(n, i, j)
    got = c.cluster(hv, n2, 21, th)
    assert_same(got, want)
    if th == 99.0:  # chained clusters and singletons side by side
        sizes = np.bincount(got[1])
        assert (sizes == 1).any() and (sizes > 2).any()


# ---- hg_cluster_dev on the bench's clustered HVs ----------------------------------------------------------------------
def clustered(n, dev):
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import bench
    hv = bench.clustered_hvs(n, 0, dev)
    return hv, (hv.int() ** 2).sum(1).int()


def hits_components(c, hv, n2, n, th, cap):
    import torch
    while True:
        out = torch.empty(cap * 3, dtype=torch.int32, device=hv.device)
        torch.cuda.synchronize()
        found, st = c.dist_dev(hv.data_ptr(), n2.data_ptr(), n, hv.data_ptr(), n2.data_ptr(), n, hv.shape[1], 21, True, th,
                               out.data_ptr(), cap)
        if st == 0:
            break
        cap = found
    h = out[: 3 * found].cpu().numpy().view(np.uint32).reshape(-1, 3)
    return model(n, h[:, 0], h[:, 1]), found


def cluster_dev(c, hv, n2, n, th):
    import torch
    rep = torch.empty(n, dtype=torch.int32, device=hv.device)
    cl = torch.empty(n, dtype=torch.int32, device=hv.device)
    torch.cuda.synchronize()
    nc = c.cluster_dev(hv.data_ptr(), n2.data_ptr(), n, hv.shape[1], rep.data_ptr(), cl.data_ptr(), 21, th)
    return rep.cpu().numpy().view(np.uint32), cl.cpu().numpy().view(np.uint32), nc


@pytest.mark.parametrize("th", [85.0, 95.0])
def test_cluster_dev_clustered_10k(gctx, th):
    import torch
    c, hg, dev = gctx
    n = 10_000
    hv, n2 = clustered(n, dev)
    want, found = hits_components(c, hv, n2, n, th, 4_000_000)
    assert found > 100_000
    assert_same(cluster_dev(c, hv, n2, n, th), want)
    try:
        c.set_debug("pair_limit", str(2_000_000))  # row blocks of a few hundred rows
        assert_same(cluster_dev(c, hv, n2, n, th), want)
    finally:
        c.set_debug("pair_limit", "0")
    try:
        c.set_debug("cluster_hit_cap", "1000")  # the scratch list overflows and grows
        assert_same(cluster_dev(c, hv, n2, n, th), want)
        c.set_debug("pair_limit", str(5_000_000))
        assert_same(cluster_dev(c, hv, n2, n, th), want)
    finally:
        c.set_debug("cluster_hit_cap", "0")
        c.set_debug("pair_limit", "0")
    s = torch.cuda.current_stream(dev)
    c.set_stream(s.cuda_stream)
    try:
        assert_same(cluster_dev(c, hv, n2, n, th), want)
    finally:
        c.reset_stream()


def test_cluster_dev_beyond_2_32_pairs(gctx):
    c, hg, dev = gctx
    n = 100_000
    assert n * (n - 1) // 2 > 2 ** 32  # the symmetric comparison cannot be one launch: row blocks
    hv, n2 = clustered(n, dev)
    want, found = hits_components(c, hv, n2, n, 85.0, 8_000_000)
    assert found > 4_000_000
    got = cluster_dev(c, hv, n2, n, 85.0)
    assert_same(got, want)
    del hv, n2


# ---- command line ------------------------------------------------------------------------------------------------------
def write_fasta(path, seq, name):
    s = bytes(seq).decode()
    with open(path, "w") as f:
        f.write(">%s\n" % name)
        for i in range(0, len(s), 80):
            f.write(s[i:i + 80] + "\n")


def test_cli_cluster_end_to_end(tmp_path):
    import hypergen_amd as hg
    from oracle import oracle as orc
    orc.lib()
    d = tmp_path / "fa"
    d.mkdir()
    ids = [0, 3, 9, 40, 99, 100, 101, 150, 300]  # cluster roots 0, 1, 3 with members at several distances
    for g in ids:
        write_fasta(str(d / ("g%03d.fna" % g)), orc.synth_genome(g, 200_000)[1:], "g%d" % g)
    sk = str(tmp_path / "all.sketch")
    r = subprocess.run([hg.CLI_PATH, "sketch", "-p", str(d), "-o", sk, "-s", "100", "-t", "4"], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr
    files = [x["file_str"] for x in hg.read_sketch_file(sk)]
    # model: oracle sketches of the same files, the oracle's ANI matrix, components over i < j
    hvs, n2s = [], []
    for f in files:
        hv, n2, _ = orc.sketch_genome(hg.read_merge_seq(f), ksize=21, scaled=100, norm=orc.NORM_U2T)
        hvs.append(hv), n2s.append(n2)
    hvs, n2s = np.stack(hvs), np.array(n2s, np.int32)
    ani = orc.ani_matrix(hvs, n2s, hvs, n2s, 21)
    i, j = np.nonzero(np.triu(ani >= np.float32(95.0), 1))
    rep, cl, nc = model(len(files), i, j)
    want = "".join("%s\t%d\t%s\n" % (files[k], cl[k], files[rep[k]]) for k in range(len(files))).encode()
    assert 1 < nc < len(files)

    out = str(tmp_path / "clusters.tsv")
    r = subprocess.run([hg.CLI_PATH, "cluster", "-p", sk, "-o", out, "-a", "95"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    got = open(out, "rb").read()
    assert got == want
    singletons = int((np.bincount(cl) == 1).sum())
    assert ("Output %d genomes in %d clusters (%d singletons) at ANI threshold 95.0 to file %s" % (len(files), nc, singletons, out)
            in r.stdout)
    assert "Clustered %d files took" % len(files) in r.stdout
    # 95.0 is the subcommand's default; two runs give the same bytes
    out2 = str(tmp_path / "clusters2.tsv")
    r = subprocess.run([hg.CLI_PATH, "cluster", "-p", sk, "-o", out2], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert open(out2, "rb").read() == got
    # the same components as the pairs `dist` reports at the same threshold
    tsv = str(tmp_path / "ani.tsv")
    r = subprocess.run([hg.CLI_PATH, "dist", "-r", sk, "-q", sk, "-o", tsv, "-a", "95"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    idx = {f: k for k, f in enumerate(files)}
    pairs = [l.split("\t")[:2] for l in open(tsv).read().splitlines()]
    rep2, cl2, nc2 = model(len(files), [idx[p[0]] for p in pairs], [idx[p[1]] for p in pairs])
    assert nc2 == nc and np.array_equal(rep2, rep) and np.array_equal(cl2, cl)
