"""Greedy representative clustering on the device (hg_cluster_greedy*, `hyper-gen cluster --linkage greedy`): rep, cluster,
ani and the cluster count EQUAL, bit for bit, to the sequential definition of tests/cluster_greedy_ref.py -- on constructed
hit lists (the worst case of the round loop, stars, ties, thresholds at the float boundary; one round per readback and
the default), on real sketches against the oracle's ANI matrix under both symmetric metrics, on the bench's clustered HVs
against the hits of hg_dist_dev (row blocks that cut through groups, the grow path, a borrowed stream) with the two
invariants checked directly on the full matrix, through the host form and end to end through the command line."""
import os
import subprocess
import sys

import numpy as np
import pytest

import cluster_greedy_ref as gr
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
    for key in ("greedy_rounds", "pair_limit", "cluster_hit_cap"):
        c.set_debug(key, "0")
    c.set_ani_metric(cr.MASH)


def run_hits(gctx, n, h, th, with_ani=True):
    """hg_cluster_greedy_hits_dev on the hit array h -> numpy (rep, cluster, ani, count)"""
    import torch
    c, hg, dev = gctx
    rep = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    cl = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    ani = torch.empty(max(n, 1), dtype=torch.float32, device=dev)
    d = torch.from_numpy(h.view(np.uint8).copy()).to(dev) if h is not None and h.size else None
    torch.cuda.synchronize()  # (the ctx runs on its own stream)
    nc = c.cluster_greedy_hits_dev(n, d.data_ptr() if d is not None else None, h.size if h is not None else 0, th, rep.data_ptr(),
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
    c.set_debug("greedy_rounds", "1")
    one = run_hits(gctx, n, h, th)
    c.set_debug("greedy_rounds", "0")
    dflt = run_hits(gctx, n, h, th)
    assert_same(one, dflt)
    return dflt, c.cluster_greedy_rounds()


# ---- constructed hit lists ---------------------------------------------------------------------------------------------
def test_chain_of_three_differs_from_single_linkage(gctx):
    import torch
    c, hg, dev = gctx
    h = hits_array([0, 1], [1, 2], [96.0, 97.0])
    got, _ = both(gctx, 3, h, 95.0)
    assert_same(got, gr.greedy_model(3, [0, 1], [1, 2], [96.0, 97.0], 95.0))
    assert got[0].tolist() == [0, 0, 2] and got[3] == 2
    rep = torch.empty(3, dtype=torch.int32, device=dev)
    cl = torch.empty(3, dtype=torch.int32, device=dev)
    d = torch.from_numpy(h.view(np.uint8).copy()).to(dev)
    torch.cuda.synchronize()
    c.cluster_init_dev(rep.data_ptr(), 3)
    c.cluster_add_hits_dev(rep.data_ptr(), 3, d.data_ptr(), 2, 95.0)
    assert c.cluster_finish_dev(rep.data_ptr(), 3, cl.data_ptr()) == 1  # single linkage: one component
    assert rep.cpu().tolist() == [0, 0, 0]


def test_ascending_path_is_the_worst_case(gctx):
    n = 2001
    k = np.arange(n - 1, dtype=np.uint32)
    ani = (95.0 + (k % 50) * 0.1).astype(np.float32)
    got, rounds = both(gctx, n, hits_array(k, k + 1, ani), 95.0)
    assert_same(got, gr.greedy_model(n, k, k + 1, ani, 95.0))
    idx = np.arange(n, dtype=np.uint32)
    assert np.array_equal(got[0], idx - (idx & 1))  # representatives: the even indices; 2k + 1 belongs to 2k
    assert got[3] == 1001
    assert rounds >= 1000


def test_descending_path_with_orientations_duplicates_and_self_pairs(gctx):
    n = 2001
    k = np.arange(n - 2, -1, -1, dtype=np.uint32)
    ani = (95.0 + (k % 50) * 0.1).astype(np.float32)
    want = gr.greedy_model(n, k, k + 1, ani, 95.0)
    a = np.concatenate([k + 1, k[::3], k[::5], k[::7]])       # reversed, forward, duplicates (a lower ANI), self-pairs
    b = np.concatenate([k, k[::3] + 1, k[::5] + 1, k[::7]])
    v = np.concatenate([ani, ani[::3], ani[::5] - np.float32(0.05), np.full(k[::7].size, 100.0, np.float32)])
    got, rounds = both(gctx, n, hits_array(a, b, v), 95.0)
    assert_same(got, want)
    assert_same(got, gr.greedy_model(n, a, b, v, 95.0))
    assert rounds >= 1000


def test_star_on_the_last_index(gctx):
    n = 1000
    leaves = np.arange(n - 1, dtype=np.uint32)
    centre = np.full(n - 1, n - 1, np.uint32)
    ani = np.random.default_rng(2).permutation(np.linspace(95.5, 99.5, n - 1).astype(np.float32))
    assert np.unique(ani).size == n - 1
    got, rounds = both(gctx, n, hits_array(centre, leaves, ani), 95.0)
    assert_same(got, gr.greedy_model(n, centre, leaves, ani, 95.0))
    assert got[3] == n - 1 and np.array_equal(got[0][:-1], leaves)  # every leaf is a representative
    assert got[0][-1] == int(np.argmax(ani)) and got[2][-1] == ani.max()
    got, _ = both(gctx, n, hits_array(centre, leaves, 97.0), 95.0)  # all equal: the smallest index
    assert got[0][-1] == 0 and got[3] == n - 1 and got[2][-1] == np.float32(97.0)


def test_star_on_index_zero(gctx):
    n = 1000
    k = np.arange(1, n, dtype=np.uint32)
    ani = np.random.default_rng(4).uniform(95.0, 100.0, n - 1).astype(np.float32)
    got, rounds = both(gctx, n, hits_array(k, np.zeros(n - 1, np.uint32), ani), 95.0)
    assert got[3] == 1 and not got[0].any() and not got[1].any()
    assert got[2][0] == np.float32(100.0) and np.array_equal(got[2][1:], ani)
    assert rounds == 2


def test_threshold_boundary_and_one_list_at_two_thresholds(gctx):
    th = np.float32(95.0)
    below = np.nextafter(th, np.float32(0))
    a = np.array([0, 2, 4, 6], np.uint32)
    b = np.array([1, 3, 5, 7], np.uint32)
    ani = np.array([th, below, th, below], np.float32)
    got, _ = both(gctx, 8, hits_array(a, b, ani), float(th))
    assert_same(got, gr.greedy_model(8, a, b, ani, float(th)))
    assert got[0].tolist() == [0, 0, 2, 3, 4, 4, 6, 7] and got[3] == 6
    got, _ = both(gctx, 8, hits_array(a, b, ani), float(below))
    assert_same(got, gr.greedy_model(8, a, b, ani, float(below)))
    assert got[0].tolist() == [0, 0, 2, 2, 4, 4, 6, 6] and got[3] == 4
    assert got[2].view(np.uint32).tolist() == np.array([100, th, 100, below, 100, th, 100, below], np.float32).view(np.uint32).tolist()


def test_member_keeps_its_earlier_representative(gctx):
    # 1 joins 0 at 96; 2 is a representative within 99 of 1: it does not take 1 over.  3 is nearer to 2 than to 0.
    a, b, v = [0, 1, 0, 2], [1, 2, 3, 3], [96.0, 99.0, 96.5, 98.0]
    got, _ = both(gctx, 4, hits_array(a, b, v), 95.0)
    assert_same(got, gr.greedy_model(4, a, b, v, 95.0))
    assert got[0].tolist() == [0, 0, 2, 2] and got[2].tolist() == [100.0, 96.0, 100.0, 98.0]


def test_random_sparse_graph(gctx):
    rng = np.random.default_rng(11)
    n, m = 20_000, 100_000
    a = rng.integers(0, n, m, dtype=np.uint32)
    b = rng.integers(0, n, m, dtype=np.uint32)
    ani = rng.uniform(80.0, 100.0, m).astype(np.float32)
    got, rounds = both(gctx, n, hits_array(a, b, ani), 95.0)
    assert_same(got, gr.greedy_model(n, a, b, ani, 95.0))
    assert 1 < got[3] < n


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
    got, rounds = both(gctx, n, hits_array(a[p], b[p], ani[p]), 95.0)
    assert_same(got, gr.greedy_model(n, a, b, ani, 95.0))
    assert groups < got[3] < n
    assert rounds <= 50


def test_empty_single_and_null_ani(gctx):
    c, hg, dev = gctx
    assert c.cluster_greedy_hits_dev(0, None, 0, 95.0, None, None) == 0  # n = 0
    got = run_hits(gctx, 1, hits_array([0], [0], [100.0]), 95.0)
    assert_same(got, (np.zeros(1, np.uint32), np.zeros(1, np.uint32), np.full(1, 100.0, np.float32), 1))
    for h in (None, hits_array([], [], [])):  # an empty list: everybody is a representative
        got = run_hits(gctx, 1000, h, 95.0)
        idx = np.arange(1000, dtype=np.uint32)
        assert_same(got, (idx, idx, np.full(1000, 100.0, np.float32), 1000))
        assert c.cluster_greedy_rounds() == 1
    h = hits_array([0, 1], [1, 2], [96.0, 97.0])
    assert_same(run_hits(gctx, 3, h, 95.0, with_ani=False), gr.greedy_model(3, [0, 1], [1, 2], [96.0, 97.0], 95.0), with_ani=False)


def test_index_out_of_range_is_invalid(gctx):
    c, hg, dev = gctx
    with pytest.raises(hg.HgError) as e:
        run_hits(gctx, 100, hits_array([1, 3], [2, 100], [99.0, 99.0]), 95.0)
    assert e.value.status == hg.ERR_INVALID
    # the next call on the ctx starts clean; a bad index below the threshold is an error too
    assert run_hits(gctx, 100, hits_array([1], [2], [99.0]), 95.0)[3] == 99
    with pytest.raises(hg.HgError):
        run_hits(gctx, 100, hits_array([1], [5000], [10.0]), 95.0)
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


def single_linkage_count(ani, th):
    reach = (ani >= np.float32(th)) | np.eye(ani.shape[0], dtype=bool)
    while True:
        nxt = (reach.astype(np.int32) @ reach.astype(np.int32)) > 0
        if np.array_equal(nxt, reach):
            return np.unique(reach, axis=0).shape[0]
        reach = nxt


@pytest.mark.parametrize("metric", [cr.MASH, cr.MAX_CONTAINMENT])
@pytest.mark.parametrize("th", [85.0, 95.0, 99.0, 99.9])
def test_real_sketches_against_oracle(gctx, real_sketches, th, metric):
    """The recipe's own order puts each root first, and member m lies m * 0.1 % from its root: whoever is within th of any
    member is within th of the root, so every component is a star on its first node and the greedy rule cuts nothing
    (at 99: 182 clusters both ways under mash, 181 under max containment).  The same sketches are therefore resolved a
    second time in descending order, far members first, and it is there that the chains must show: at 99, more clusters
    than single linkage gives on the same matrix (191 against 182, 190 against 181)."""
    c, hg, dev = gctx
    hv, n2, mats = real_sketches
    c.set_ani_metric(metric)
    assert_same(c.cluster_greedy(hv, n2, 21, th), gr.greedy_model_matrix(mats[metric], th))
    p = np.arange(hv.shape[0])[::-1]
    m = np.ascontiguousarray(mats[metric][np.ix_(p, p)])
    want = gr.greedy_model_matrix(m, th)
    assert_same(c.cluster_greedy(np.ascontiguousarray(hv[p]), np.ascontiguousarray(n2[p]), 21, th), want)
    if th == 99.0:  # chains that single linkage joins and the greedy rule cuts: otherwise this shows nothing
        print("greedy %d clusters, single linkage %d" % (want[3], single_linkage_count(m, th)))
        assert want[3] > single_linkage_count(m, th)


def test_directional_metric_is_invalid(gctx, real_sketches):
    c, hg, dev = gctx
    hv, n2, mats = real_sketches
    c.set_ani_metric(cr.CONTAINMENT)
    with pytest.raises(hg.HgError) as e:
        c.cluster_greedy(hv, n2, 21, 95.0)
    assert e.value.status == hg.ERR_INVALID
    assert "HG_ANI_CONTAINMENT is directional" in str(e.value)


# ---- hg_cluster_greedy_dev on the bench's clustered HVs ----------------------------------------------------------------
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


def greedy_dev(c, hv, n2, th):
    import torch
    rep = torch.empty(N_BENCH, dtype=torch.int32, device=hv.device)
    cl = torch.empty(N_BENCH, dtype=torch.int32, device=hv.device)
    ani = torch.empty(N_BENCH, dtype=torch.float32, device=hv.device)
    torch.cuda.synchronize()
    nc = c.cluster_greedy_dev(hv.data_ptr(), n2.data_ptr(), N_BENCH, hv.shape[1], rep.data_ptr(), cl.data_ptr(), ani.data_ptr(), 21, th)
    torch.cuda.synchronize()
    return rep.cpu().numpy().view(np.uint32), cl.cpu().numpy().view(np.uint32), ani.cpu().numpy(), nc


@pytest.mark.parametrize("where", ["95", "median"])
def test_greedy_dev_clustered(gctx, clustered, where):
    import torch
    c, hg, dev = gctx
    hv, n2, full, median = clustered
    th = 95.0 if where == "95" else median
    a, b, v = dist_hits(c, hv, n2, th)
    want = gr.greedy_model(N_BENCH, a, b, v, th)
    got = greedy_dev(c, hv, n2, th)
    assert_same(got, want)
    if where == "median":
        assert got[3] > 30
    # the two invariants, directly on the full matrix
    reps = np.flatnonzero(got[0] == np.arange(N_BENCH))
    sub = full[np.ix_(reps, reps)]
    assert (sub[~np.eye(reps.size, dtype=bool)] < np.float32(th)).all()
    m = np.flatnonzero(got[0] != np.arange(N_BENCH))
    assert (got[0][m] < m).all() and np.isin(got[0][m], reps).all()
    assert (full[got[0][m], m] >= np.float32(th)).all()
    assert np.array_equal(full[got[0][m], m].view(np.uint32), got[2][m].view(np.uint32))
    assert (got[2][reps] == np.float32(100.0)).all()
    # row blocks (one row per block; blocks that cut through groups), the grow path, both, a borrowed stream
    for limit, cap in (("3000", "0"), ("20000", "0"), ("500000", "0"), ("0", "100"), ("20000", "100")):
        c.set_debug("pair_limit", limit)
        c.set_debug("cluster_hit_cap", cap)
        assert_same(greedy_dev(c, hv, n2, th), want)
    c.set_debug("pair_limit", "0")
    c.set_debug("cluster_hit_cap", "0")
    c.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    try:
        assert_same(greedy_dev(c, hv, n2, th), want)
    finally:
        c.reset_stream()


def test_host_form_equals_dev_form(gctx, clustered):
    import torch
    c, hg, dev = gctx
    hv, n2, full, median = clustered
    n = 500
    h_hv, h_n2 = hv[:n].cpu().numpy(), n2[:n].cpu().numpy()
    rep = torch.empty(n, dtype=torch.int32, device=dev)
    cl = torch.empty(n, dtype=torch.int32, device=dev)
    ani = torch.empty(n, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    nc = c.cluster_greedy_dev(hv.data_ptr(), n2.data_ptr(), n, hv.shape[1], rep.data_ptr(), cl.data_ptr(), ani.data_ptr(), 21, median)
    torch.cuda.synchronize()
    want = (rep.cpu().numpy().view(np.uint32), cl.cpu().numpy().view(np.uint32), ani.cpu().numpy(), nc)
    assert_same(c.cluster_greedy(h_hv, h_n2, 21, median), want)
    assert_same(want, gr.greedy_model_matrix(full[:n, :n], median))
    assert 5 < nc < n


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


def test_cli_greedy_end_to_end(tmp_path):
    import hypergen_amd as hg
    from oracle import oracle as orc
    orc.lib()
    d = tmp_path / "fa"
    d.mkdir()
    ids = [0, 3, 9, 40, 99, 100, 101, 150, 300]  # cluster roots 0, 1, 3 with members at several distances
    for g in ids:
        write_fasta(str(d / ("g%03d.fna" % g)), orc.synth_genome(g, 200_000)[1:], "g%d" % g)
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

    def lines(perm):
        """the model on the matrix in processing order perm, written in file order"""
        rep, cl, v, nc = gr.greedy_model_matrix(ani[np.ix_(perm, perm)], 95.0)
        pos = np.argsort(perm)
        return "".join("%s\t%d\t%s\t%.3f\n" % (files[i], cl[pos[i]], files[perm[rep[pos[i]]]], float(v[pos[i]]))
                       for i in range(n)).encode(), cl, nc

    want, cl, nc = lines(np.arange(n))
    assert 1 < nc < n
    out = str(tmp_path / "greedy.tsv")
    r = cli(hg, "cluster", "-p", sk, "-o", out, "-a", "95", "--linkage", "greedy")
    got = open(out, "rb").read()
    assert got == want
    singletons = int((np.bincount(cl) == 1).sum())
    assert ("Output %d genomes in %d clusters (%d singletons) at ANI threshold 95.0 to file %s" % (n, nc, singletons, out)) in r.stdout
    assert "Clustered %d files took" % n in r.stdout
    # --order file is the default
    out2 = str(tmp_path / "greedy_file.tsv")
    cli(hg, "cluster", "-p", sk, "-o", out2, "--linkage", "greedy", "--order", "file")
    assert open(out2, "rb").read() == want
    # --linkage single writes what no flag writes
    o_none, o_single = str(tmp_path / "none.tsv"), str(tmp_path / "single.tsv")
    r_none = cli(hg, "cluster", "-p", sk, "-o", o_none, "-a", "95")
    r_single = cli(hg, "cluster", "-p", sk, "-o", o_single, "-a", "95", "--linkage", "single")
    assert open(o_none, "rb").read() == open(o_single, "rb").read() != got
    assert all(len(l.split("\t")) == 3 for l in open(o_single).read().splitlines())
    assert "Output %d genomes in" % n in r_single.stdout and "Clustered %d files took" % n in r_single.stdout
    # --order size: descending hv_norm_2, ties in file order; the lines stay in file order
    perm = np.argsort(-n2s.astype(np.int64), kind="stable")
    assert not np.array_equal(perm, np.arange(n))
    want_size, _, nc_size = lines(perm)
    out3 = str(tmp_path / "greedy_size.tsv")
    cli(hg, "cluster", "-p", sk, "-o", out3, "-a", "95", "--linkage", "greedy", "--order", "size")
    got_size = open(out3, "rb").read()
    assert got_size == want_size
    assert [l.split(b"\t")[0].decode() for l in got_size.splitlines()] == files
    # the ANI column is the ANI field `dist` writes for the same pair
    tsv = str(tmp_path / "ani.tsv")
    cli(hg, "dist", "-r", sk, "-q", sk, "-o", tsv, "-a", "95")
    field = {}
    for l in open(tsv).read().splitlines():
        r_, q_, v_ = l.split("\t")
        field[(r_, q_)] = field[(q_, r_)] = v_
    members = 0
    for text in (got, got_size):
        for l in text.decode().splitlines():
            f, _, rf, v = l.split("\t")
            if f == rf:
                assert v == "100.000"
            else:
                assert field[(f, rf)] == v
                members += 1
    assert members > 0
