"""Greedy set-cover clustering on the device (hg_cluster_setcover*, `hyper-gen cluster --linkage setcover`): rep, cluster,
ani and the cluster count EQUAL, bit for bit, to the sequential definition of tests/cluster_setcover_ref.py -- on
constructed hit lists (the hand cases of the surface test, the worst case of the round loop, stars, a random graph, partial
cliques; one round per readback and the default), on real sketches against the oracle's ANI matrix under both symmetric
metrics, on the bench's clustered HVs against the hits of hg_dist_dev (row blocks, the append-and-grow path of the hit
list, a borrowed stream) with the two invariants checked directly on the full matrix, through the host form and end to end
through the command line."""
import os
import subprocess
import sys

import numpy as np
import pytest

import cluster_greedy_ref as gr
import cluster_setcover_ref as sc
import containment_ref as cr

pytestmark = pytest.mark.gpu


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


@pytest.fixture(autouse=True)
def clean_hooks(gctx):
    yield
    c = gctx[0]
    for key in ("setcover_rounds", "pair_limit", "cluster_hit_cap"):
        c.set_debug(key, "0")
    c.set_ani_metric(cr.MASH)


def run_hits(gctx, n, h, th, with_ani=True):
    """hg_cluster_setcover_hits_dev on the hit array h -> numpy (rep, cluster, ani, count)"""
    import torch
    c, hg, dev = gctx
    rep = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    cl = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    ani = torch.empty(max(n, 1), dtype=torch.float32, device=dev)
    d = torch.from_numpy(h.view(np.uint8).copy()).to(dev) if h is not None and h.size else None
    torch.cuda.synchronize()  # (the ctx runs on its own stream)
    nc = c.cluster_setcover_hits_dev(n, d.data_ptr() if d is not None else None, h.size if h is not None else 0, th, rep.data_ptr(),
                                     cl.data_ptr(), ani.data_ptr() if with_ani else None)
    return rep[:n].cpu().numpy().view(np.uint32), cl[:n].cpu().numpy().view(np.uint32), ani[:n].cpu().numpy(), nc


def assert_same(got, want, with_ani=True):
    assert got[3] == want[3], "cluster count"
    assert np.array_equal(got[0], want[0]), "rep"
    assert np.array_equal(got[1], want[1]), "cluster"
    if with_ani:
        assert np.array_equal(got[2].view(np.uint32), want[2].view(np.uint32)), "ani"


def both(gctx, n, h, th):
    """the list resolved with one round per readback and with the default: the same result; -> (result, rounds of the default run)"""
    c = gctx[0]
    c.set_debug("setcover_rounds", "1")
    one = run_hits(gctx, n, h, th)
    rounds_one = c.cluster_setcover_rounds()
    c.set_debug("setcover_rounds", "0")
    dflt = run_hits(gctx, n, h, th)
    assert_same(one, dflt)
    assert c.cluster_setcover_rounds() == rounds_one  # (the rounds queued behind the last one do not count)
    return dflt, rounds_one


def against_model(gctx, n, a, b, ani, th):
    got, rounds = both(gctx, n, hits_array(a, b, ani), th)
    want = sc.setcover_model(n, a, b, ani, th)
    assert_same(got, want)
    return got, rounds


def edges(*stars):
    a, b, v = [], [], []
    for centre, leaves, ani in stars:
        for leaf in leaves:
            a.append(centre), b.append(leaf), v.append(ani)
    return np.array(a, np.uint32), np.array(b, np.uint32), np.array(v, np.float32)


# ---- constructed hit lists ---------------------------------------------------------------------------------------------
def test_chain_of_three_is_one_cluster(gctx):
    got, rounds = against_model(gctx, 3, [0, 1], [1, 2], [97.0, 97.0], 95.0)
    assert got[0].tolist() == [1, 1, 1] and got[3] == 1 and rounds == 1
    assert gr.greedy_model(3, [0, 1], [1, 2], [97.0, 97.0], 95.0)[3] == 2


def test_four_cycle(gctx):
    got, rounds = against_model(gctx, 4, [0, 1, 2, 3], [1, 2, 3, 0], [97.0] * 4, 95.0)
    assert got[0].tolist() == [0, 0, 2, 0] and rounds == 2


def test_degrees_are_recounted(gctx):
    a, b, v = edges((0, [1, 2, 3, 4, 5], 97.0), (6, [3, 4, 5, 7], 97.0), (8, [9, 10, 11], 97.0), (7, [12, 13], 97.0))
    got, _ = against_model(gctx, 14, a, b, v, 95.0)
    assert got[0].tolist() == [0, 0, 0, 0, 0, 0, 7, 7, 8, 8, 8, 8, 7, 7]


def test_two_stars_sharing_a_leaf(gctx):
    a, b, v = edges((0, [1, 2, 3, 4, 5, 6], 96.0), (10, [6], 99.0), (10, [11, 12, 13, 14], 96.0))
    got, _ = against_model(gctx, 15, a, b, v, 95.0)
    assert got[0].tolist() == [0, 0, 0, 0, 0, 0, 0, 7, 8, 9, 10, 10, 10, 10, 10]
    assert got[2][6] == np.float32(96.0)


def test_duplicate_with_a_higher_ani_behind_the_lower_one(gctx):
    # the pair (1, 2) three times: whatever the order of the records, the member carries the highest ANI
    a, b, v = [0, 1, 2, 1], [1, 2, 1, 2], [96.0, 95.5, 98.5, 97.0]
    got, _ = against_model(gctx, 3, a, b, v, 95.0)
    assert got[0].tolist() == [1, 1, 1] and got[2].tolist() == [96.0, 100.0, 98.5]


def path_lists(order):
    """every pair (k, k + 1) of the path twice -- forward and, interleaved, reversed with a lower ANI -- and a self-pair of
    every seventh node"""
    n = 2001
    k = np.arange(n - 1, dtype=np.uint32)[::order]
    ani = (95.1 + (k % 50) * 0.1).astype(np.float32)  # (the duplicates, 0.05 lower, stay above the threshold: every pair counts twice)
    a = np.stack([k, k + 1], 1).ravel()
    b = np.stack([k + 1, k], 1).ravel()
    v = np.stack([ani, ani - np.float32(0.05)], 1).ravel()
    s = k[::7]
    return n, np.concatenate([a, s]), np.concatenate([b, s]), np.concatenate([v, np.full(s.size, 100.0, np.float32)]), k, ani


@pytest.mark.parametrize("order", [1, -1], ids=["ascending", "descending"])
def test_path_is_the_worst_case(gctx, order):
    n, a, b, v, k, ani = path_lists(order)
    got, rounds = against_model(gctx, n, a, b, v, 95.0)
    idx = np.arange(n)
    assert np.array_equal(got[0], np.minimum(3 * (idx // 3) + 1, 2000))  # every third node, and the last one for the tail
    assert got[3] == 667
    assert rounds >= 667
    assert_same(got, sc.setcover_model(n, k, k + 1, ani, 95.0))  # every pair twice resolves like every pair once


def test_star_on_the_last_index(gctx):
    n = 1000
    leaves = np.arange(n - 1, dtype=np.uint32)
    centre = np.full(n - 1, n - 1, np.uint32)
    ani = np.random.default_rng(2).permutation(np.linspace(95.5, 99.5, n - 1).astype(np.float32))
    got, rounds = against_model(gctx, n, centre, leaves, ani, 95.0)
    assert got[3] == 1 and (got[0] == n - 1).all() and not got[1].any()
    assert np.array_equal(got[2][:-1], ani) and got[2][-1] == np.float32(100.0)  # the leaves carry their own ANI
    assert rounds == 1
    assert gr.greedy_model(n, centre, leaves, ani, 95.0)[3] == n - 1


def test_threshold_boundary(gctx):
    th = np.float32(95.0)
    below = np.nextafter(th, np.float32(0))
    a, b, v = [0, 2, 4, 6], [1, 3, 5, 7], [th, below, th, np.nan]
    got, _ = against_model(gctx, 8, a, b, v, float(th))
    assert got[0].tolist() == [0, 0, 2, 3, 4, 4, 6, 7] and got[3] == 6
    got, _ = against_model(gctx, 8, a, b, v, float(below))
    assert got[0].tolist() == [0, 0, 2, 2, 4, 4, 6, 7] and got[3] == 5  # (NaN never counts)
    assert got[2].view(np.uint32).tolist() == np.array([100, th, 100, below, 100, th, 100, 100], np.float32).view(np.uint32).tolist()


def test_random_sparse_graph(gctx):
    rng = np.random.default_rng(11)
    n, m = 20_000, 100_000
    a = rng.integers(0, n, m, dtype=np.uint32)
    b = rng.integers(0, n, m, dtype=np.uint32)
    ani = rng.uniform(80.0, 100.0, m).astype(np.float32)
    got, rounds = against_model(gctx, n, a, b, ani, 95.0)
    assert 1 < got[3] < n
    print("random sparse graph: %d clusters in %d rounds" % (got[3], rounds))


def test_partial_cliques(gctx):
    rng = np.random.default_rng(17)
    groups, size = 200, 50
    n = groups * size
    i, j = np.triu_indices(size, 1)
    a, b = [], []
    for g in range(groups):
        keep = rng.random(i.size) < 0.5  # half of each group's pairs
        a.append(g * size + i[keep]), b.append(g * size + j[keep])
    a, b = np.concatenate(a).astype(np.uint32), np.concatenate(b).astype(np.uint32)
    ani = rng.uniform(95.0, 100.0, a.size).astype(np.float32)
    p = rng.permutation(a.size)
    got, rounds = against_model(gctx, n, a[p], b[p], ani[p], 95.0)
    assert groups < got[3] < n
    print("partial cliques: %d clusters in %d rounds" % (got[3], rounds))
    assert rounds <= 50


def test_empty_single_and_null_ani(gctx):
    c, hg, dev = gctx
    assert c.cluster_setcover_hits_dev(0, None, 0, 95.0, None, None) == 0  # n = 0
    got = run_hits(gctx, 1, hits_array([0], [0], [100.0]), 95.0)
    assert_same(got, (np.zeros(1, np.uint32), np.zeros(1, np.uint32), np.full(1, 100.0, np.float32), 1))
    for h in (None, hits_array([], [], [])):  # a NULL list, an empty list: everybody is a representative
        got = run_hits(gctx, 1000, h, 95.0)
        idx = np.arange(1000, dtype=np.uint32)
        assert_same(got, (idx, idx, np.full(1000, 100.0, np.float32), 1000))
        assert c.cluster_setcover_rounds() == 1
    h = hits_array([0, 1], [1, 2], [96.0, 97.0])
    assert_same(run_hits(gctx, 3, h, 95.0, with_ani=False), sc.setcover_model(3, [0, 1], [1, 2], [96.0, 97.0], 95.0), with_ani=False)


def test_index_out_of_range_is_invalid(gctx):
    c, hg, dev = gctx
    with pytest.raises(hg.HgError) as e:
        run_hits(gctx, 100, hits_array([1, 3], [2, 100], [99.0, 99.0]), 95.0)
    assert e.value.status == hg.ERR_INVALID
    # the next call on the ctx starts clean; a bad index below the threshold is an error too
    assert run_hits(gctx, 100, hits_array([1], [2], [99.0]), 95.0)[3] == 99
    with pytest.raises(hg.HgError) as e:
        run_hits(gctx, 100, hits_array([1], [5000], [10.0]), 95.0)
    assert e.value.status == hg.ERR_INVALID
    assert run_hits(gctx, 100, hits_array([1], [2], [99.0]), 95.0)[3] == 99


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
    """the host form on the recipe's own order and on the reversed one, against the model on the oracle's matrix"""
    c, hg, dev = gctx
    hv, n2, mats = real_sketches
    c.set_ani_metric(metric)
    want = sc.setcover_model_matrix(mats[metric], th)
    assert_same(c.cluster_setcover(hv, n2, 21, th), want)
    p = np.arange(hv.shape[0])[::-1]
    m = np.ascontiguousarray(mats[metric][np.ix_(p, p)])
    want_rev = sc.setcover_model_matrix(m, th)
    assert_same(c.cluster_setcover(np.ascontiguousarray(hv[p]), np.ascontiguousarray(n2[p]), 21, th), want_rev)
    print("th %.1f metric %d: %d set-cover clusters, %d reversed, %d greedy" % (th, metric, want[3], want_rev[3],
                                                                                gr.greedy_model_matrix(mats[metric], th)[3]))


def test_directional_metric_is_invalid(gctx, real_sketches):
    c, hg, dev = gctx
    hv, n2, mats = real_sketches
    c.set_ani_metric(cr.CONTAINMENT)
    with pytest.raises(hg.HgError) as e:
        c.cluster_setcover(hv, n2, 21, 95.0)
    assert e.value.status == hg.ERR_INVALID
    assert "HG_ANI_CONTAINMENT is directional" in str(e.value)


# ---- hg_cluster_setcover_dev on the bench's clustered HVs -------------------------------------------------------------
N_BENCH = 3_000


@pytest.fixture(scope="module")
def clustered(gctx):
    """(hv, n2, full ANI matrix on the host, median within-cluster ANI of rows 0..299)"""
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


def dist_hits(c, hv, n2, th):
    import torch
    cap = 400_000
    while True:
        out = torch.empty(cap * 3, dtype=torch.int32, device=hv.device)
        torch.cuda.synchronize()
        found, st = c.dist_dev(hv.data_ptr(), n2.data_ptr(), N_BENCH, hv.data_ptr(), n2.data_ptr(), N_BENCH, hv.shape[1], 21, True, th,
                               out.data_ptr(), cap)
        if st == 0:
            break
        cap = found
    h = out[: 3 * found].cpu().numpy()
    return h.view(np.uint32).reshape(-1, 3)[:, 0], h.view(np.uint32).reshape(-1, 3)[:, 1], h.view(np.float32).reshape(-1, 3)[:, 2]


def setcover_dev(c, hv, n2, th, n=N_BENCH):
    import torch
    rep = torch.empty(n, dtype=torch.int32, device=hv.device)
    cl = torch.empty(n, dtype=torch.int32, device=hv.device)
    ani = torch.empty(n, dtype=torch.float32, device=hv.device)
    torch.cuda.synchronize()
    nc = c.cluster_setcover_dev(hv.data_ptr(), n2.data_ptr(), n, hv.shape[1], rep.data_ptr(), cl.data_ptr(), ani.data_ptr(), 21, th)
    torch.cuda.synchronize()
    return rep.cpu().numpy().view(np.uint32), cl.cpu().numpy().view(np.uint32), ani.cpu().numpy(), nc


@pytest.mark.parametrize("where", ["95", "median"])
def test_setcover_dev_clustered(gctx, clustered, where):
    import torch
    c, hg, dev = gctx
    hv, n2, full, median = clustered
    th = 95.0 if where == "95" else median
    a, b, v = dist_hits(c, hv, n2, th)
    want = sc.setcover_model(N_BENCH, a, b, v, th)
    got = setcover_dev(c, hv, n2, th)
    assert_same(got, want)
    print("clustered at %s: %d hits, %d clusters in %d rounds" % (where, a.size, got[3], c.cluster_setcover_rounds()))
    if where == "median":
        assert got[3] > 30
    # the two invariants, directly on the full matrix
    idx = np.arange(N_BENCH)
    reps = np.flatnonzero(got[0] == idx)
    sub = full[np.ix_(reps, reps)]
    assert (sub[~np.eye(reps.size, dtype=bool)] < np.float32(th)).all()
    m = np.flatnonzero(got[0] != idx)
    assert np.isin(got[0][m], reps).all()
    assert (full[got[0][m], m] >= np.float32(th)).all()
    assert np.array_equal(full[got[0][m], m].view(np.uint32), got[2][m].view(np.uint32))
    assert (got[2][reps] == np.float32(100.0)).all()
    # row blocks (one row per block; blocks that cut through groups), the append-and-grow path of the list across several
    # blocks, both, a borrowed stream
    for limit, cap in (("3000", "0"), ("20000", "0"), ("500000", "0"), ("0", "100"), ("20000", "100")):
        c.set_debug("pair_limit", limit)
        c.set_debug("cluster_hit_cap", cap)
        assert_same(setcover_dev(c, hv, n2, th), want)
    c.set_debug("pair_limit", "0")
    c.set_debug("cluster_hit_cap", "0")
    c.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    try:
        assert_same(setcover_dev(c, hv, n2, th), want)
    finally:
        c.reset_stream()


def test_host_form_equals_dev_form(gctx, clustered):
    c, hg, dev = gctx
    hv, n2, full, median = clustered
    n = 500
    h_hv, h_n2 = hv[:n].cpu().numpy(), n2[:n].cpu().numpy()
    want = setcover_dev(c, hv, n2, median, n)
    assert_same(c.cluster_setcover(h_hv, h_n2, 21, median), want)
    assert_same(want, sc.setcover_model_matrix(full[:n, :n], median))
    assert 5 < want[3] < n


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


def test_cli_setcover_end_to_end(gctx, tmp_path):
    c, hg, dev = gctx
    from oracle import oracle as orc
    orc.lib()
    d = tmp_path / "fa"
    d.mkdir()
    # the far members come first in the file: the representatives set cover chooses are not the first of their groups
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
    assert n2s.tolist() == [x["hv_norm_2"] for x in recs]
    ani = orc.ani_matrix(hvs, n2s, hvs, n2s, 21)

    def four_columns(rep, cl, v):
        return "".join("%s\t%d\t%s\t%.3f\n" % (files[i], cl[i], files[rep[i]], float(v[i])) for i in range(n)).encode()

    rep, cl, v, nc = sc.setcover_model_matrix(ani, 95.0)
    assert 1 < nc < n and (rep > np.arange(n)).any()
    out = str(tmp_path / "setcover.tsv")
    r = cli(hg, "cluster", "-p", sk, "-o", out, "-a", "95", "--linkage", "setcover")
    got = open(out, "rb").read()
    assert got == four_columns(rep, cl, v)
    singletons = int((np.bincount(cl) == 1).sum())
    assert ("Output %d genomes in %d clusters (%d singletons) at ANI threshold 95.0 to file %s" % (n, nc, singletons, out)) in r.stdout
    assert "Clustered %d files took" % n in r.stdout
    # the other linkages write what the existing calls give on the same sketches
    g_rep, g_cl, g_v, g_nc = c.cluster_greedy(hvs, n2s, 21, 95.0)
    o_greedy = str(tmp_path / "greedy.tsv")
    cli(hg, "cluster", "-p", sk, "-o", o_greedy, "-a", "95", "--linkage", "greedy")
    assert open(o_greedy, "rb").read() == four_columns(g_rep, g_cl, g_v) != got
    s_rep, s_cl, s_nc = c.cluster(hvs, n2s, 21, 95.0)
    want_single = "".join("%s\t%d\t%s\n" % (files[i], s_cl[i], files[s_rep[i]]) for i in range(n)).encode()
    o_none, o_single = str(tmp_path / "none.tsv"), str(tmp_path / "single.tsv")
    cli(hg, "cluster", "-p", sk, "-o", o_none, "-a", "95")
    cli(hg, "cluster", "-p", sk, "-o", o_single, "-a", "95", "--linkage", "single")
    assert open(o_none, "rb").read() == open(o_single, "rb").read() == want_single
    # the ANI column is the ANI field `dist` writes for the same pair
    tsv = str(tmp_path / "ani.tsv")
    cli(hg, "dist", "-r", sk, "-q", sk, "-o", tsv, "-a", "95")
    field = {}
    for l in open(tsv).read().splitlines():
        r_, q_, v_ = l.split("\t")
        field[(r_, q_)] = field[(q_, r_)] = v_
    members = 0
    for l in got.decode().splitlines():
        f, _, rf, val = l.split("\t")
        if f == rf:
            assert val == "100.000"
        else:
            assert field[(f, rf)] == val
            members += 1
    assert members > 0
