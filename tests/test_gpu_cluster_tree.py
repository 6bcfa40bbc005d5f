"""The single-linkage tree on the device (hg_cluster_tree*, `hyper-gen cluster --tree / --levels`): the tree, rep, cluster and
the counts EQUAL, indices and ANI bit patterns, to Kruskal under the definition's order (tests/cluster_tree_ref.py) -- on
constructed hit lists (ties that would close a cycle under inconsistent tie-breaking, paths, stars, a messy list, thresholds
at the float boundary, a random list in two shuffles; one round per readback and the default, the same bytes), the cut
property through the existing step calls, on the bench's clustered HVs against the hits of hg_dist_dev (row blocks down to
one row, the grow path, a borrowed stream), on real sketches against the oracle's ANI matrix under both symmetric metrics,
through the host form and end to end through the command line."""
import os
import subprocess
import sys

import numpy as np
import pytest

import cluster_tree_ref as tr
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
    for key in ("tree_rounds", "pair_limit", "cluster_hit_cap"):
        c.set_debug(key, "0")
    c.set_ani_metric(cr.MASH)


def to_dev(gctx, h):
    import torch
    return torch.from_numpy(h.view(np.uint8).copy()).to(gctx[2]) if h is not None and h.size else None


def run_hits(gctx, n, h, th, with_clusters=True):
    """hg_cluster_tree_hits_dev on the hit array h -> (tree, rep, cluster, count) as numpy"""
    import torch
    c, hg, dev = gctx
    rep = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    cl = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    tree = torch.full((3 * max(n - 1, 1),), -1, dtype=torch.int32, device=dev)
    d = to_dev(gctx, h)
    torch.cuda.synchronize()  # (the ctx runs on its own stream)
    ne, nc = c.cluster_tree_hits_dev(n, d.data_ptr() if d is not None else None, h.size if h is not None else 0, th, tree.data_ptr(),
                                     max(n - 1, 0), rep.data_ptr() if with_clusters else None, cl.data_ptr() if with_clusters else None)
    t = tree[:3 * ne].cpu().numpy().view(np.uint8).view(hg.ANI_HIT_DTYPE)
    if not with_clusters:
        return t, None, None, nc
    return t, rep[:n].cpu().numpy().view(np.uint32), cl[:n].cpu().numpy().view(np.uint32), nc


def assert_same(got, want):
    assert got[3] == want[3], "cluster count"
    assert got[0].size == want[0].size, "tree edges"
    assert got[0].tobytes() == want[0].tobytes(), "tree"
    if got[1] is not None:
        assert np.array_equal(got[1], want[1]), "rep"
        assert np.array_equal(got[2], want[2]), "cluster"


def both(gctx, n, h, th):
    """the list resolved with one round per readback and with the default: the same bytes; -> (result, rounds of the default run)"""
    c = gctx[0]
    c.set_debug("tree_rounds", "1")
    one = run_hits(gctx, n, h, th)
    rounds_one = c.cluster_tree_rounds()
    c.set_debug("tree_rounds", "0")
    dflt = run_hits(gctx, n, h, th)
    assert_same(one, dflt)
    assert c.cluster_tree_rounds() == rounds_one  # (the rounds queued behind the one that found nothing do not count)
    assert dflt[0].size == n - dflt[3]
    return dflt, rounds_one


def cut_dev(gctx, n, d_hits, n_hits, t):
    """the existing step calls on a device hit list at threshold t -> (rep, cluster, count)"""
    import torch
    c, hg, dev = gctx
    rep = torch.empty(n, dtype=torch.int32, device=dev)
    cl = torch.empty(n, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    c.cluster_init_dev(rep.data_ptr(), n)
    if n_hits:
        c.cluster_add_hits_dev(rep.data_ptr(), n, d_hits.data_ptr(), n_hits, t)
    nc = c.cluster_finish_dev(rep.data_ptr(), n, cl.data_ptr())
    return rep.cpu().numpy().view(np.uint32), cl.cpu().numpy().view(np.uint32), nc


def assert_cuts(gctx, n, tree, full, levels):
    """the step calls on the tree == the step calls on the full list, at every level"""
    d_tree, d_full = to_dev(gctx, tree), to_dev(gctx, full)
    counts = []
    for t in levels:
        a = cut_dev(gctx, n, d_tree, tree.size, t)
        b = cut_dev(gctx, n, d_full, full.size, t)
        assert a[2] == b[2] and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), t
        counts.append(a[2])
    return counts


# ---- constructed hit lists ---------------------------------------------------------------------------------------------
def test_triangle_loses_its_weakest_edge(gctx):
    a, b, v = [0, 1, 0], [1, 2, 2], [97.0, 99.0, 96.0]
    got, _ = both(gctx, 3, hits_array(a, b, v), 95.0)
    assert_same(got, tr.tree_model(3, a, b, v, 95.0))
    assert got[0]["ref_idx"].tolist() == [1, 0] and got[0]["qry_idx"].tolist() == [2, 1] and got[0]["ani"].tolist() == [99.0, 97.0]
    assert got[3] == 1


def test_k64_with_every_ani_equal_is_the_star_on_node_0(gctx):
    i, j = np.triu_indices(64, 1)
    p = np.random.default_rng(1).permutation(i.size)
    got, rounds = both(gctx, 64, hits_array(j[p], i[p], 97.0), 95.0)
    assert_same(got, tr.tree_model(64, i, j, np.float32(97.0), 95.0))
    assert got[0]["ref_idx"].tolist() == [0] * 63 and got[0]["qry_idx"].tolist() == list(range(1, 64))
    assert rounds == 2  # every node selects an edge into 0 and 0 selects (0, 1) back; then nothing is left


def test_ring_with_every_ani_equal(gctx):
    n = 1000
    k = np.arange(n, dtype=np.uint32)
    got, rounds = both(gctx, n, hits_array(k, (k + 1) % n, 98.0), 95.0)
    assert_same(got, tr.tree_model(n, k, (k + 1) % n, np.float32(98.0), 95.0))
    pairs = list(zip(got[0]["ref_idx"].tolist(), got[0]["qry_idx"].tolist()))
    want = sorted((min(x, (x + 1) % n), max(x, (x + 1) % n)) for x in range(n))
    want.remove((998, 999))
    assert pairs == want and got[3] == 1
    assert rounds <= 11


@pytest.mark.parametrize("descending", [False, True])
def test_paths(gctx, descending):
    n = 2001
    k = np.arange(n - 1, dtype=np.uint32)
    ani = np.linspace(95.0, 99.9, n - 1).astype(np.float32)
    assert np.unique(ani).size == n - 1
    if descending:
        ani = ani[::-1].copy()
    got, rounds = both(gctx, n, hits_array(k, k + 1, ani), 95.0)
    assert_same(got, tr.tree_model(n, k, k + 1, ani, 95.0))
    order = np.argsort(-ani.astype(np.float64), kind="stable")
    assert got[0]["ref_idx"].tolist() == k[order].tolist() and got[0]["ani"].tobytes() == ani[order].tobytes()  # all edges, in ANI order
    assert got[3] == 1 and rounds <= 12


def test_stars(gctx):
    n = 1000
    leaves = np.arange(1, n, dtype=np.uint32)
    ani = np.random.default_rng(4).choice(np.linspace(95.0, 100.0, 11).astype(np.float32), n - 1)
    got, rounds = both(gctx, n, hits_array(leaves, np.zeros(n - 1, np.uint32), ani), 95.0)  # on index 0
    assert_same(got, tr.tree_model(n, leaves, np.zeros(n - 1, np.uint32), ani, 95.0))
    assert got[3] == 1 and not got[1].any() and rounds == 2
    leaves = np.arange(n - 1, dtype=np.uint32)
    centre = np.full(n - 1, n - 1, np.uint32)
    got, rounds = both(gctx, n, hits_array(centre, leaves, ani), 95.0)  # on the last index
    assert_same(got, tr.tree_model(n, centre, leaves, ani, 95.0))
    assert got[3] == 1 and (got[0]["qry_idx"] == n - 1).all() and rounds == 2


def test_messy_list_gives_the_clean_lists_tree(gctx):
    rng = np.random.default_rng(7)
    n, m = 3000, 9000
    a, b = rng.integers(0, n, m, dtype=np.uint32), rng.integers(0, n, m, dtype=np.uint32)
    keep = a != b
    a, b = a[keep], b[keep]
    v = rng.choice(np.linspace(95.0, 100.0, 21).astype(np.float32), a.size)
    want = tr.tree_model(n, a, b, v, 95.0)
    s = np.arange(0, n, 7, dtype=np.uint32)
    ma = np.concatenate([b[::2], a[1::2], a[::3], b[::5], a[::4], s])  # both orientations, duplicates with a lower ANI,
    mb = np.concatenate([a[::2], b[1::2], b[::3], a[::5], b[::4], s])  # exact duplicates (one reversed), self-pairs
    mv = np.concatenate([v[::2], v[1::2], v[::3] - np.float32(0.25), v[::5], v[::4], np.full(s.size, 100.0, np.float32)])
    p = rng.permutation(ma.size)
    got, _ = both(gctx, n, hits_array(ma[p], mb[p], mv[p]), 95.0)
    assert_same(got, want)
    assert_same(got, tr.tree_model(n, ma, mb, mv, 95.0))
    assert 1 < got[3] < n


def test_threshold_side(gctx):
    th = np.float32(95.0)
    below = np.nextafter(th, np.float32(0))
    a = np.array([0, 2, 4, 6], np.uint32)
    b = np.array([1, 3, 5, 7], np.uint32)
    ani = np.array([th, below, th, below], np.float32)
    got, _ = both(gctx, 8, hits_array(a, b, ani), float(th))
    assert_same(got, tr.tree_model(8, a, b, ani, float(th)))
    assert got[1].tolist() == [0, 0, 2, 3, 4, 4, 6, 7] and got[3] == 6 and got[0]["ref_idx"].tolist() == [0, 4]
    got, _ = both(gctx, 8, hits_array(a, b, ani), float(below))
    assert_same(got, tr.tree_model(8, a, b, ani, float(below)))
    assert got[1].tolist() == [0, 0, 2, 2, 4, 4, 6, 6] and got[3] == 4
    assert got[0]["ani"].view(np.uint32).tolist() == np.array([th, th, below, below], np.float32).view(np.uint32).tolist()
    # NaN never counts; negative ANIs and both zeros order as floats
    a, b, v = [0, 1, 2, 0], [1, 2, 3, 3], np.array([np.nan, -0.0, -1.5, 0.0], np.float32)
    got, _ = both(gctx, 4, hits_array(a, b, v), -2.0)
    assert_same(got, tr.tree_model(4, a, b, v, -2.0))
    assert got[0]["ref_idx"].tolist() == [0, 1, 2] and got[0]["qry_idx"].tolist() == [3, 2, 3]


@pytest.fixture(scope="module")
def random_list():
    rng = np.random.default_rng(11)
    n, m = 20_000, 100_000
    a = rng.integers(0, n, m, dtype=np.uint32)
    b = rng.integers(0, n, m, dtype=np.uint32)
    v = rng.choice(np.linspace(90.0, 100.0, 41).astype(np.float32), m)
    return n, a, b, v, tr.tree_model(n, a, b, v, 95.0), rng


def test_random_list_in_two_shuffles(gctx, random_list):
    n, a, b, v, want, rng = random_list
    kept = tr.counting_edges(n, a, b, v, 95.0)[0].size
    assert want[0].size == 19_890 and 50_000 < kept < 53_000  # (the seed-11 draw)
    got1, rounds = both(gctx, n, hits_array(a, b, v), 95.0)
    assert_same(got1, want)
    p = rng.permutation(a.size)
    got2, _ = both(gctx, n, hits_array(b[p], a[p], v[p]), 95.0)
    assert_same(got2, want)
    assert got1[0].tobytes() == got2[0].tobytes()
    assert 1 < got1[3] < n and got1[0].size < kept
    assert rounds <= 16  # ceil(log2 n) + 1
    assert_same(run_hits(gctx, n, hits_array(a, b, v), 95.0, with_clusters=False), want)  # the tree alone


def test_cut_property_on_the_random_list(gctx, random_list):
    n, a, b, v, want, rng = random_list
    one = np.float32(97.5)
    assert (v == one).any()
    levels = [95.0, 96.25, float(one), float(np.nextafter(one, np.float32(200))), 99.75]
    counts = assert_cuts(gctx, n, want[0], hits_array(a, b, v), levels)
    assert counts[0] == want[3] and counts == sorted(counts) and counts[2] < counts[3] < counts[4] < n


# ---- degenerate and error cases ----------------------------------------------------------------------------------------
def test_empty_single_none_and_null_pair(gctx):
    c, hg, dev = gctx
    assert c.cluster_tree_hits_dev(0, None, 0, 95.0, None, 0) == (0, 0)  # n = 0
    got = run_hits(gctx, 1, hits_array([0], [0], [100.0]), 95.0)
    assert got[0].size == 0 and got[1].tolist() == [0] and got[2].tolist() == [0] and got[3] == 1
    idx = np.arange(1000, dtype=np.uint32)
    for h in (None, hits_array([], [], []), hits_array([1, 5], [2, 5], [94.0, 100.0])):  # nothing counts: every node its own cluster
        got = run_hits(gctx, 1000, h, 95.0)
        assert got[0].size == 0 and np.array_equal(got[1], idx) and np.array_equal(got[2], idx) and got[3] == 1000
    a, b, v = [0, 1], [1, 2], [96.0, 97.0]
    got = run_hits(gctx, 4, hits_array(a, b, v), 95.0, with_clusters=False)
    assert_same(got, tr.tree_model(4, a, b, v, 95.0))
    assert got[3] == 2
    import torch
    rep = torch.empty(4, dtype=torch.int32, device=dev)
    tree = torch.empty(9, dtype=torch.int32, device=dev)
    d = to_dev(gctx, hits_array(a, b, v))
    torch.cuda.synchronize()
    with pytest.raises(hg.HgError) as e:  # rep without cluster
        c.cluster_tree_hits_dev(4, d.data_ptr(), 2, 95.0, tree.data_ptr(), 3, rep.data_ptr(), None)
    assert e.value.status == hg.ERR_INVALID
    with pytest.raises(hg.HgError) as e:  # no tree
        c.cluster_tree_hits_dev(4, d.data_ptr(), 2, 95.0, None, 3, None, None)
    assert e.value.status == hg.ERR_INVALID


def test_tree_cap_too_small_is_capacity(gctx):
    import ctypes as C
    import torch
    c, hg, dev = gctx
    n = 100
    tree = torch.full((3 * n,), -1, dtype=torch.int32, device=dev)
    d = to_dev(gctx, hits_array([1], [2], [99.0]))
    torch.cuda.synchronize()
    ne, nc = C.c_size_t(7), C.c_size_t(7)
    st = hg.lib().hg_cluster_tree_hits_dev(c._h, n, C.c_void_p(d.data_ptr()), 1, C.c_float(95.0), C.c_void_p(tree.data_ptr()), n - 2,
                                           C.byref(ne), None, None, C.byref(nc))
    assert st == hg.ERR_CAPACITY and ne.value == n - 1 and nc.value == 0
    torch.cuda.synchronize()
    assert (tree.cpu().numpy() == -1).all()  # nothing launched
    with pytest.raises(hg.HgError) as e:
        c.cluster_tree_hits_dev(n, d.data_ptr(), 1, 95.0, tree.data_ptr(), n - 2)
    assert e.value.status == hg.ERR_CAPACITY
    assert c.cluster_tree_hits_dev(n, d.data_ptr(), 1, 95.0, tree.data_ptr(), n - 1) == (1, n - 1)


def test_index_out_of_range_is_invalid(gctx):
    c, hg, dev = gctx
    with pytest.raises(hg.HgError) as e:
        run_hits(gctx, 100, hits_array([1, 3], [2, 100], [99.0, 99.0]), 95.0)
    assert e.value.status == hg.ERR_INVALID
    # the next call on the ctx starts clean; a bad index below the threshold is an error too
    assert run_hits(gctx, 100, hits_array([1], [2], [99.0]), 95.0)[3] == 99
    with pytest.raises(hg.HgError):
        run_hits(gctx, 100, hits_array([1], [5000], [10.0]), 95.0)
    got = run_hits(gctx, 100, hits_array([1], [2], [99.0]), 95.0)
    assert got[3] == 99 and got[0].size == 1


# ---- hg_cluster_tree_dev on the bench's clustered HVs ------------------------------------------------------------------
N_BENCH = 3_000


@pytest.fixture(scope="module")
def clustered(gctx):
    """(hv, n2, median within-cluster ANI of rows 0..299)"""
    import torch
    c, hg, dev = gctx
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import bench
    hv = bench.clustered_hvs(N_BENCH, 0, dev)
    n2 = (hv.int() ** 2).sum(1).int()
    full = torch.empty(300 * 300, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    c.dist_full_dev(hv.data_ptr(), n2.data_ptr(), 300, hv.data_ptr(), n2.data_ptr(), 300, hv.shape[1], 21, full.data_ptr())
    c.sync()
    full = full.cpu().numpy().reshape(300, 300)
    i, j = np.triu_indices(300, 1)
    within = full[i, j][i // 100 == j // 100]  # (clustered_hvs: groups of 100 consecutive rows)
    return hv, n2, float(np.median(within))


def dist_hits(c, hg, hv, n2, th):
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
    return out[: 3 * found].cpu().numpy().view(np.uint8).view(hg.ANI_HIT_DTYPE).copy()


def tree_dev(gctx, hv, n2, n, th):
    import torch
    c, hg, dev = gctx
    rep = torch.empty(n, dtype=torch.int32, device=dev)
    cl = torch.empty(n, dtype=torch.int32, device=dev)
    tree = torch.full((3 * (n - 1),), -1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    ne, nc = c.cluster_tree_dev(hv.data_ptr(), n2.data_ptr(), n, hv.shape[1], tree.data_ptr(), n - 1, rep.data_ptr(), cl.data_ptr(), 21, th)
    torch.cuda.synchronize()
    return tree[:3 * ne].cpu().numpy().view(np.uint8).view(hg.ANI_HIT_DTYPE), rep.cpu().numpy().view(np.uint32), cl.cpu().numpy().view(np.uint32), nc


@pytest.mark.parametrize("where", ["95", "median"])
def test_tree_dev_clustered(gctx, clustered, where):
    import torch
    c, hg, dev = gctx
    hv, n2, median = clustered
    th = 95.0 if where == "95" else median
    h = dist_hits(c, hg, hv, n2, th)
    want = tr.tree_model(N_BENCH, h["ref_idx"], h["qry_idx"], h["ani"], th)
    got = tree_dev(gctx, hv, n2, N_BENCH, th)
    assert_same(got, want)
    assert got[0].size == N_BENCH - got[3] < h.size
    if where == "median":
        assert 30 < got[3] < N_BENCH
    # rep / cluster / count are hg_cluster_dev's
    rep = torch.empty(N_BENCH, dtype=torch.int32, device=dev)
    cl = torch.empty(N_BENCH, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    nc = c.cluster_dev(hv.data_ptr(), n2.data_ptr(), N_BENCH, hv.shape[1], rep.data_ptr(), cl.data_ptr(), 21, th)
    torch.cuda.synchronize()
    assert nc == got[3] and np.array_equal(rep.cpu().numpy().view(np.uint32), got[1]) and np.array_equal(cl.cpu().numpy().view(np.uint32), got[2])
    # the cut property: five thresholds that include an edge's ANI and the float after it
    edge = got[0]["ani"][got[0].size // 2]  # (an edge's own ANI)
    levels = [th, float(edge), float(np.nextafter(edge, np.float32(200))), float(got[0]["ani"].max()), 100.0]
    counts = assert_cuts(gctx, N_BENCH, got[0], h, sorted(levels))
    assert counts[0] == got[3] and counts == sorted(counts) and counts[0] < counts[-1]
    # row blocks (one row per block; blocks that cut through groups), the grow path, both, a borrowed stream
    for limit, cap in (("3000", "0"), ("20000", "0"), ("500000", "0"), ("0", "100"), ("20000", "100")):
        c.set_debug("pair_limit", limit)
        c.set_debug("cluster_hit_cap", cap)
        assert_same(tree_dev(gctx, hv, n2, N_BENCH, th), want)
    c.set_debug("pair_limit", "0")
    c.set_debug("cluster_hit_cap", "0")
    c.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    try:
        assert_same(tree_dev(gctx, hv, n2, N_BENCH, th), want)
    finally:
        c.reset_stream()


def test_host_form_equals_dev_form(gctx, clustered):
    c, hg, dev = gctx
    hv, n2, median = clustered
    n = 500
    want = tree_dev(gctx, hv, n2, n, median)
    got = c.cluster_tree(hv[:n].cpu().numpy(), n2[:n].cpu().numpy(), 21, median)
    assert_same(got, want)
    assert 5 < got[3] < n
    alone = c.cluster_tree(hv[:n].cpu().numpy(), n2[:n].cpu().numpy(), 21, median, want_clusters=False)
    assert alone[1] is None and alone[2] is None
    assert_same(alone, want)


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
    c, hg, dev = gctx
    hv, n2, mats = real_sketches
    c.set_ani_metric(metric)
    want = tr.tree_model_matrix(mats[metric], th)
    assert_same(c.cluster_tree(hv, n2, 21, th), want)
    rep, cl, nc = c.cluster(hv, n2, 21, th)
    assert nc == want[3] and np.array_equal(rep, want[1]) and np.array_equal(cl, want[2])


def test_directional_metric_is_invalid(gctx, real_sketches):
    c, hg, dev = gctx
    hv, n2, mats = real_sketches
    c.set_ani_metric(cr.CONTAINMENT)
    with pytest.raises(hg.HgError) as e:
        c.cluster_tree(hv, n2, 21, 95.0)
    assert e.value.status == hg.ERR_INVALID
    assert "HG_ANI_CONTAINMENT is directional" in str(e.value)


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


def test_cli_tree_and_levels_end_to_end(tmp_path):
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
    ani = orc.ani_matrix(hvs, n2s, hvs, n2s, 21)
    floor = 92.0
    tree, rep, cl, nc = tr.tree_model_matrix(ani, floor)
    assert 1 < nc < n and tree.size == n - nc
    cuts = [(rep, cl, nc)] + [tr.cut(n, tree, t) for t in (97.0, 99.0)]
    assert cuts[0][2] < cuts[2][2]  # the levels tell something apart
    want_tree = "".join("%s\t%s\t%.3f\n" % (files[e["ref_idx"]], files[e["qry_idx"]], float(e["ani"])) for e in tree).encode()
    want_out = "".join("\t".join([files[i]] + [x for r_, c_, _ in cuts for x in (str(c_[i]), files[r_[i]])]) + "\n" for i in range(n)).encode()
    out, tf = str(tmp_path / "levels.tsv"), str(tmp_path / "tree.tsv")
    r = cli(hg, "cluster", "-p", sk, "-o", out, "-a", "92", "--tree", tf, "--levels", "97,99")
    assert open(tf, "rb").read() == want_tree
    got = open(out, "rb").read()
    assert got == want_out
    for (r_, c_, k), name in zip(cuts, ("92.0", "97.0", "99.0")):
        singletons = int((np.bincount(c_) == 1).sum())
        assert ("Output %d genomes in %d clusters (%d singletons) at ANI threshold %s to file %s" % (n, k, singletons, name, out)) in r.stdout
    assert r.stdout.count("Output %d genomes in" % n) == 3
    # level columns are nested: equal id at 99 => equal id at 97 => equal id at -a
    rows = [l.split("\t") for l in got.decode().splitlines()]
    assert all(len(x) == 1 + 2 * 3 for x in rows)
    for x in rows:
        for y in rows:
            if x[5] == y[5]:
                assert x[3] == y[3]
            if x[3] == y[3]:
                assert x[1] == y[1]
    # --tree alone: the usual three columns, the same tree; --levels alone: the same columns, no tree file
    o2, t2 = str(tmp_path / "plain.tsv"), str(tmp_path / "tree2.tsv")
    cli(hg, "cluster", "-p", sk, "-o", o2, "-a", "92", "--tree", t2, "--linkage", "single")
    assert open(t2, "rb").read() == want_tree
    o_none, o_single = str(tmp_path / "none.tsv"), str(tmp_path / "single.tsv")
    cli(hg, "cluster", "-p", sk, "-o", o_none, "-a", "92")
    cli(hg, "cluster", "-p", sk, "-o", o_single, "-a", "92", "--linkage", "single")
    assert open(o_none, "rb").read() == open(o_single, "rb").read() == open(o2, "rb").read()
    assert open(o_none, "rb").read() == b"".join(b"\t".join(l.split(b"\t")[:3]) + b"\n" for l in got.splitlines())
    # the tree's ANI fields are the ones `dist` writes for the same pairs
    tsv = str(tmp_path / "ani.tsv")
    cli(hg, "dist", "-r", sk, "-q", sk, "-o", tsv, "-a", "92")
    field = {}
    for l in open(tsv).read().splitlines():
        r_, q_, v_ = l.split("\t")
        field[(r_, q_)] = field[(q_, r_)] = v_
    lines = open(tf).read().splitlines()
    assert len(lines) == n - nc
    for l in lines:
        a, b, v = l.split("\t")
        assert field[(a, b)] == v


def test_cli_levels_without_tree(gctx, tmp_path):
    """--levels alone: the tree is built for its cuts only and no tree file is written.  16 sketches at hv_d 1024 (a cluster of 8,
    half of another, 4 loners); the bytes of -o are those of hg_cluster_tree and of the step calls on its edges (cut_dev), formatted
    as test_cli_tree_and_levels_end_to_end formats them; the levels are two of the tree's own ANIs, written so that the command
    line reads back the same float32"""
    import bench
    c, hg, dev = gctx
    n, hv_d, floor = 16, 1024, 93.0

    def rows(m, first):
        return bench.clustered_hvs(m, first, dev, n=900, cluster=8).cpu().numpy()[:, :hv_d].copy()

    hv = np.concatenate([rows(12, 0)] + [rows(1, 1000 + 8 * j) for j in range(4)])
    n2 = cr.norms(hv)
    files = ["/d/%sg%02d.fna" % ("x" * (i % 3), i) for i in range(n)]
    recs = []
    for i in range(n):
        q, pk = hg.hv_pack(hv[i])
        recs.append(dict(ksize=21, scaled=1500, canonical=True, seed=123, hv_d=hv_d, hv_quant_bits=q, hv_norm_2=int(n2[i]),
                         file_str=files[i], hv=pk.view(np.int16)))
    sk, out = str(tmp_path / "sixteen.sketch"), str(tmp_path / "levels.tsv")
    hg.write_sketch_file(sk, recs)
    tree, rep, cl, nc = c.cluster_tree(hv, n2, 21, floor)
    assert nc == 6 and tree.size == n - nc
    anis = np.unique(tree["ani"])
    lo, hi = float(anis[anis.size // 2]), float(anis[-1])
    assert floor < lo < hi
    d_tree = to_dev(gctx, tree)
    cuts = [(rep, cl, nc)] + [cut_dev(gctx, n, d_tree, tree.size, t) for t in (lo, hi)]
    assert nc < cuts[1][2] < cuts[2][2] < n  # the levels tell something apart; the strongest edge reaches the last one
    want = "".join("\t".join([files[i]] + [x for r_, c_, _ in cuts for x in (str(c_[i]), files[r_[i]])]) + "\n" for i in range(n)).encode()
    r = cli(hg, "cluster", "-p", sk, "-o", out, "-a", "%.9g" % floor, "--levels", "%.9g,%.9g" % (lo, hi))
    assert open(out, "rb").read() == want
    assert sorted(os.listdir(str(tmp_path))) == ["levels.tsv", "sixteen.sketch"]
    for (r_, c_, k), t in zip(cuts, (floor, lo, hi)):
        name = "%.1f" % t if np.float32("%.1f" % t) == np.float32(t) else "%g" % t  # (as the log line prints a level)
        singletons = int((np.bincount(c_) == 1).sum())
        assert ("Output %d genomes in %d clusters (%d singletons) at ANI threshold %s to file %s" % (n, k, singletons, name, out)) in r.stdout
    assert r.stdout.count("Output %d genomes in" % n) == 3
