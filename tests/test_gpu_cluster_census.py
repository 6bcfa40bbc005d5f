"""Every clustering, tree and statistics kernel (tests/cluster_census.py), run through the entry its census row names at a
small input that makes the row's kernel show in the result, against the Python models (cluster_tree_ref.components,
cluster_greedy_ref, cluster_setcover_ref, cluster_tree_ref, cluster_average_ref, cluster_complete_ref, cluster_stats_ref,
nj_ref); and the finishing kernels every scheme shares -- tiles of 1024 nodes -- on graphs whose roots sit on the tile border.

Every comparison is `==` on integers or on the bits of floats.  Where a call reports rounds or counts they are asserted: the
number a model gives, or the one derived next to the input.  Output buffers are pre-filled with 0x5A bytes.
"""
import numpy as np
import pytest
import torch

import cluster_average_ref as av
import cluster_census as cc
import cluster_complete_ref as cp
import cluster_greedy_ref as gr
import cluster_setcover_ref as sv
import cluster_stats_ref as st
import cluster_tree_ref as tr
import containment_ref as cr
import nj_ref as nj

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = 0x5A
D = 4096
HIT = np.dtype([("ref_idx", "<u4"), ("qry_idx", "<u4"), ("ani", "<f4")])


@pytest.fixture(scope="module")
def hg():
    import hypergen_amd
    return hypergen_amd


@pytest.fixture(scope="module")
def mctx(hg):
    c = hg.Context(0)
    # (the ctx's own stream does not wait for torch's: the sentinel fills and uploads below must be in front of the kernels)
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    yield c
    c.close()


@pytest.fixture
def ctx(mctx):
    yield mctx
    mctx.set_debug("pair_limit", "0")
    mctx.set_ani_metric(cr.MASH)


def out_buf(nbytes):
    return torch.full((max(int(nbytes), 1) + 64,), SENT, dtype=torch.uint8, device=DEV)


def host(buf, nbytes, dtype):
    h = buf.cpu().numpy()
    assert (h[nbytes:] == SENT).all(), "bytes behind the output were written"
    return h[:nbytes].copy().view(dtype)


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a).reshape(-1).view(np.uint8).copy()).to(DEV)


def hits_array(a, b, ani):
    h = np.zeros(len(a), HIT)
    h["ref_idx"], h["qry_idx"], h["ani"] = a, b, ani
    return h


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def sym(a):
    a = np.triu(np.asarray(a, np.float32), 1)
    return a + a.T


def nan_below(a):
    """the matrix with NaN on and below the diagonal: what the rounds read there is the mirror kernel's copy of the upper half"""
    b = np.array(a, np.float32)
    b[np.tril_indices(b.shape[0])] = np.nan
    return b


# ---- single linkage in steps: init, hits, finish --------------------------------------------------------------------------
def run_steps(ctx, n, parts, th, check_init=False):
    """hg_cluster_init_dev, one hg_cluster_add_hits_dev per part, hg_cluster_finish_dev -> (rep, cluster, count)"""
    rep, cl = out_buf(4 * n), out_buf(4 * n)
    ctx.cluster_init_dev(rep.data_ptr(), n)
    if check_init:
        assert np.array_equal(host(rep, 4 * n, np.uint32), np.arange(n, dtype=np.uint32))
    held = [up(h) for h in parts]  # (the calls are queued: the lists stay until the finish has read its words back)
    for h, d_h in zip(parts, held):
        ctx.cluster_add_hits_dev(rep.data_ptr(), n, d_h.data_ptr() if h.size else 0, h.size, th)
    nc = ctx.cluster_finish_dev(rep.data_ptr(), n, cl.data_ptr())
    return host(rep, 4 * n, np.uint32), host(cl, 4 * n, np.uint32), nc


def same_components(got, n, h, th):
    want = tr.components(n, h["ref_idx"], h["qry_idx"], h["ani"], th) if h.size else tr.components(n, [], [], np.zeros(0, np.float32), th)
    assert got[2] == want[2], ("cluster count", got[2], want[2])
    assert np.array_equal(got[0], want[0]), "rep"
    assert np.array_equal(got[1], want[1]), "cluster"
    return want


def split3(rng, h):
    p = rng.permutation(h.size)
    return [h[p[k::3]] for k in range(3)]


TILE_N = (1, 1023, 1024, 1025, 2049)


def tile_graph(kind, n):
    """(a) no hits; (b) the path 0 - 1 - ... - n - 1: one component; (c) the components of 0 and of 1023, 1024 and 1025 -- the
    last node of the first tile and the first two of the second (those that exist) -- as paths: 1 .. 1022 hang on 0, the nodes
    from 1026 on go to the three in turn.  (Node 0 is the smallest index of its component whatever the graph: it is always a root.)"""
    if kind == "a" or n == 1:
        return hits_array([], [], [])
    if kind == "b":
        k = np.arange(n - 1)
        return hits_array(k, k + 1, 99.0)
    a, b = [], []
    last = {0: 0, 1023: 1023, 1024: 1024, 1025: 1025}
    for i in range(1, n):
        if i in last:
            continue
        root = 0 if i < 1023 else (1023, 1024, 1025)[i % 3]
        a.append(last[root]), b.append(i)
        last[root] = i
    return hits_array(a, b, 99.0)


@pytest.mark.parametrize("kind", ["a", "b", "c"])
@pytest.mark.parametrize("n", TILE_N)
def test_finishing_kernels_on_the_tile_border(ctx, n, kind):
    rng = np.random.default_rng(n)
    h = tile_graph(kind, n)
    noise = hits_array(rng.integers(0, n, 50), rng.integers(0, n, 50), 94.9)  # below the threshold: these do not count
    got = run_steps(ctx, n, split3(rng, np.concatenate([h, noise])), 95.0, check_init=True)
    want = same_components(got, n, h, 95.0)
    roots = np.flatnonzero(got[0] == np.arange(n)).tolist()
    if kind == "a" or n == 1:
        assert roots == list(range(n)) and np.array_equal(got[1], np.arange(n)) and got[2] == n
    elif kind == "b":
        assert roots == [0] and not got[1].any() and got[2] == 1
    else:
        assert roots == [r for r in (0, 1023, 1024, 1025) if r < n] and want[2] == len(roots)
        if n == 2049:  # members of all three sit in the third tile; their ids come from roots of the first and the second
            assert set(got[0][2048:].tolist()) | set(got[0][1026:1029].tolist()) == {1023, 1024, 1025}
            assert got[1][1023] == 1 and got[1][1024] == 2 and got[1][1025] == 3 and got[1][2048] == got[1][got[0][2048]]


# ---- the runners of the rows ----------------------------------------------------------------------------------------------
def run_single_linkage(hg, ctx):
    """2500 nodes (three tiles): random pairs around the threshold in both orientations, self pairs, and a path of 300 nodes
    whose edges come in three calls and any order -- rep[] holds trees of some depth when the finish begins.  Without the hook
    every node is a root; without the compress rep[] names parents, not roots; without the scan, the root ids or the member ids
    cluster[] keeps its 0x5A bytes or the count is off"""
    n = 2500
    rng = np.random.default_rng(1)
    k = np.arange(1000, 1299)
    h = np.concatenate([hits_array(rng.integers(0, n, 1500), rng.integers(0, n, 1500), rng.uniform(90.0, 100.0, 1500).astype(np.float32)),
                        hits_array(k + 1, k, 96.0), hits_array(np.arange(50), np.arange(50), 100.0)])
    got = run_steps(ctx, n, split3(rng, h), 95.0, check_init=True)
    want = same_components(got, n, h, 95.0)
    assert 1 < want[2] < n and (got[0][1000:1300] == got[0][1000]).all()


def rep_outputs(n):
    return out_buf(4 * n), out_buf(4 * n), out_buf(4 * n)


def rep_result(bufs, n, nc):
    return host(bufs[0], 4 * n, np.uint32), host(bufs[1], 4 * n, np.uint32), host(bufs[2], 4 * n, np.float32), nc


def same_rep(got, want):
    assert got[3] == want[3], ("cluster count", got[3], want[3])
    assert np.array_equal(got[0], want[0]), "rep"
    assert np.array_equal(got[1], want[1]), "cluster"
    assert np.array_equal(bits(got[2]), bits(want[2])), "ani"


def star_hits(rng, groups, size, first=0):
    """`groups` stars: the centre is the lowest index of its group, its size - 1 leaves follow it; ANI values all different"""
    centre = first + np.repeat(np.arange(groups) * size, size - 1)
    leaf = centre + np.tile(np.arange(1, size), groups)
    ani = rng.permutation(np.linspace(95.5, 99.5, centre.size).astype(np.float32))
    return centre, leaf, ani


def run_greedy_hits(hg, ctx):
    """40 stars of 25 nodes, and two more nodes that hang on two centres each, in both orientations.  Round 1: the centres have
    no earlier neighbour and become representatives, mark blocks everybody else; round 2: mark makes them members, nobody is
    left: 2 rounds.  Without mark or decide nothing but representatives come out (or nothing ends), without assign the members
    have no best word and stay their own representatives, without rep_ani rep[] and ani[] keep their 0x5A bytes"""
    rng = np.random.default_rng(2)
    n = 1002
    a, b, v = star_hits(rng, 40, 25)
    extra = hits_array([1000, 25, 0, 1001], [0, 1000, 1001, 50], [96.0, 98.5, 97.25, 97.0])
    h = np.concatenate([hits_array(a, b, v), extra])
    h = h[rng.permutation(h.size)]
    flip = rng.random(h.size) < 0.5
    h["ref_idx"], h["qry_idx"] = np.where(flip, h["qry_idx"], h["ref_idx"]), np.where(flip, h["ref_idx"], h["qry_idx"])
    bufs = rep_outputs(n)
    d_h = up(h)
    nc = ctx.cluster_greedy_hits_dev(n, d_h.data_ptr(), h.size, 95.0, bufs[0].data_ptr(), bufs[1].data_ptr(), bufs[2].data_ptr())
    got = rep_result(bufs, n, nc)
    same_rep(got, gr.greedy_model(n, h["ref_idx"], h["qry_idx"], h["ani"], 95.0))
    assert nc == 40 and ctx.cluster_greedy_rounds() == 2
    assert got[0][1000] == 25 and got[2][1000] == np.float32(98.5) and got[0][1001] == 0 and got[2][1001] == np.float32(97.25)


_SKETCHES = {}


def sketches():
    """150 sketch-like hypervectors of graded similarity on the device, and hg_dist_full_dev's matrix of them on the host"""
    if not _SKETCHES:
        hv, _, _ = cr.fragment_hvs(150, D, seed=41)
        _SKETCHES.update(hv=up(hv), n2=up(cr.norms(hv)), n=150)
    return _SKETCHES


def run_greedy_blocks(hg, ctx):
    """hg_cluster_greedy_dev in row blocks of at most 1500 pairs.  The model on the device's own matrix names members of later
    blocks whose representative sits in an earlier one: greedy_enter_kernel has to find them covered -- it would otherwise
    leave them undecided, and their own block would make them representatives or hand them to a nearer, later one"""
    s = sketches()
    n, limit = s["n"], 1500
    m = out_buf(4 * n * n)
    ctx.dist_full_dev(s["hv"].data_ptr(), s["n2"].data_ptr(), n, s["hv"].data_ptr(), s["n2"].data_ptr(), n, D, 21, m.data_ptr())
    ani = host(m, 4 * n * n, np.float32).reshape(n, n)
    i, j = np.triu_indices(n, 1)
    th = float(np.percentile(ani[i, j], 80))
    want = gr.greedy_model_matrix(ani, th)
    starts, r0 = [], 0
    while r0 < n:  # (hg_cluster_row_blocks: rows [r0, r1) against the columns from r0 on)
        starts.append(r0)
        r0 += min(n - r0, max(1, limit // (n - r0)))
    block = np.searchsorted(np.array(starts), np.arange(n), side="right") - 1
    assert len(starts) > 4 and (block[want[0]] < block).sum() > 5
    ctx.set_debug("pair_limit", str(limit))
    bufs = rep_outputs(n)
    nc = ctx.cluster_greedy_dev(s["hv"].data_ptr(), s["n2"].data_ptr(), n, D, bufs[0].data_ptr(), bufs[1].data_ptr(), bufs[2].data_ptr(), 21, th)
    same_rep(rep_result(bufs, n, nc), want)
    assert 1 < nc < n


def run_setcover_hits(hg, ctx):
    """20 stars of 4 to 23 leaves (nodes of different degree), the pair {900, 901} given twice at 96 and at 98, and the path
    950 - 951 - ... - 956.  The stars and the pair resolve in round 1.  On the path round 1 selects 951 alone (degree 2, the
    lowest index; 953 -- two hops away -- sees its key through the second spread), round 2 selects 954 among 953 .. 956, round 3
    the node 956 that nobody covers: 3 rounds"""
    rng = np.random.default_rng(3)
    n = 1000
    a, b = [], []
    at = 0
    for g in range(20):
        a += [at] * (4 + g)
        b += list(range(at + 1, at + 5 + g))
        at += 5 + g
    assert at <= 900
    v = rng.permutation(np.linspace(95.5, 99.5, len(a)).astype(np.float32))
    k = np.arange(950, 956)
    h = np.concatenate([hits_array(a, b, v), hits_array([900, 901], [901, 900], [96.0, 98.0]), hits_array(k, k + 1, 97.0),
                        hits_array([5, 7], [5, 8], [100.0, 94.0])])  # (a self pair, a pair below the threshold)
    h = h[rng.permutation(h.size)]
    bufs = rep_outputs(n)
    d_h = up(h)
    nc = ctx.cluster_setcover_hits_dev(n, d_h.data_ptr(), h.size, 95.0, bufs[0].data_ptr(), bufs[1].data_ptr(), bufs[2].data_ptr())
    got = rep_result(bufs, n, nc)
    same_rep(got, sv.setcover_model(n, h["ref_idx"], h["qry_idx"], h["ani"], 95.0))
    assert ctx.cluster_setcover_rounds() == 3
    assert got[0][950:957].tolist() == [951, 951, 951, 954, 954, 954, 956]
    assert got[0][901] == 900 and got[2][901] == np.float32(98.0)


def run_tree_hits(hg, ctx):
    """the path 0 - 1 - ... - 399: edges {2i, 2i + 1} at 99 - i / 100, edges {2i + 1, 2i + 2} at 97 - i / 100, every edge twice
    (the second time reversed, at a lower ANI), all of them ties broken nowhere.  Round 1: both ends of every strong edge select
    it (a mutual selection, emitted once); round 2: every pair selects the weak edge to the pair in front of it (the first pair
    the one behind it) and all hook into one component; round 3 selects nothing: 3 rounds, 399 edges, one cluster"""
    n = 400
    i = np.arange(n // 2)
    strong = hits_array(2 * i, 2 * i + 1, (99.0 - i / 100.0).astype(np.float32))
    weak = hits_array(2 * i[:-1] + 1, 2 * i[:-1] + 2, (97.0 - i[:-1] / 100.0).astype(np.float32))
    h = np.concatenate([strong, weak])
    again = hits_array(h["qry_idx"], h["ref_idx"], h["ani"] - np.float32(0.5))
    h = np.concatenate([h, again])
    h = h[np.random.default_rng(4).permutation(h.size)]
    tree, rep, cl = out_buf(12 * (n - 1)), out_buf(4 * n), out_buf(4 * n)
    d_h = up(h)
    ne, nc = ctx.cluster_tree_hits_dev(n, d_h.data_ptr(), h.size, 95.0, tree.data_ptr(), n - 1, rep.data_ptr(), cl.data_ptr())
    want = tr.tree_model(n, h["ref_idx"], h["qry_idx"], h["ani"], 95.0)
    assert (ne, nc) == (n - 1, 1) == (want[0].size, want[3])
    assert np.array_equal(bits(host(tree, 12 * ne, HIT)), bits(want[0]))
    assert np.array_equal(host(rep, 4 * n, np.uint32), want[1]) and np.array_equal(host(cl, 4 * n, np.uint32), want[2])
    assert ctx.cluster_tree_rounds() == 3


def dendro_outputs(n):
    return {k: out_buf(4 * n) for k in ("rep", "cluster", "into", "level", "size")}


def dendro_result(o, n, nc):
    return tuple(host(o[k], 4 * n, np.float32 if k == "level" else np.uint32) for k in ("rep", "cluster", "into", "level", "size")) + (nc,)


def same_dendro(got, want):
    assert got[5] == want[5], ("cluster count", got[5], want[5])
    for k, name in enumerate(("rep", "cluster", "into", "level", "size")):
        assert np.array_equal(bits(got[k]), bits(want[k])), name


def linkage_matrix(seed, n=70):
    """n = 70: three mirror tiles a side, rows padded; groups of 7 with strong pairs inside, a band of values between them"""
    rng = np.random.default_rng(seed)
    a = rng.uniform(80.0, 94.0, (n, n))
    g = rng.permutation(n) % 10
    within = g[:, None] == g[None, :]
    a[within] = rng.uniform(90.0, 99.9, int(within.sum()))
    return sym(a)


def run_average_matrix(hg, ctx):
    """the upper triangle given, NaN on and below the diagonal: a best partner found in the lower half (every row's partners
    with a lower index) comes from the mirror.  Rounds and merges are the round model's; into / level / size are written by the
    emit kernel alone"""
    a = linkage_matrix(5)
    n = a.shape[0]
    want = av.average_model_rounds(a, 93.0, with_rounds=True)
    assert 1 < want[5] < n - 20 and want[6] >= 3
    o = dendro_outputs(n)
    d_a = up(nan_below(a))
    nc = ctx.cluster_average_matrix_dev(d_a.data_ptr(), n, 93.0, *(o[k].data_ptr() for k in ("rep", "cluster", "into", "level", "size")))
    same_dendro(dendro_result(o, n, nc), want)
    assert ctx.cluster_average_rounds() == want[6]


def run_complete_matrix(hg, ctx):
    """as for average linkage; three rounds or more, so that complete_best_kernel's rescan of the rows a merge invalidated runs
    (from round 2 on) and rows it leaves alone keep their partner"""
    a = linkage_matrix(6)
    n = a.shape[0]
    want = cp.complete_model_rounds(a, 91.0, with_rounds=True)
    assert 1 < want[5] < n - 20 and want[6] >= 4
    o = dendro_outputs(n)
    d_a = up(nan_below(a))
    nc = ctx.cluster_complete_matrix_dev(d_a.data_ptr(), n, 91.0, *(o[k].data_ptr() for k in ("rep", "cluster", "into", "level", "size")))
    same_dendro(dendro_result(o, n, nc), want)
    assert ctx.cluster_complete_rounds() == want[6]


def run_stats_matrix(hg, ctx):
    """70 nodes in 9 clusters of which one is empty and one a singleton, an asymmetric matrix: node and cluster records"""
    rng = np.random.default_rng(7)
    n, k = 70, 9
    a = rng.uniform(70.0, 100.0, (n, n)).astype(np.float32)
    cl = rng.integers(0, 7, n).astype(np.uint32)
    cl[cl == 3] = 4  # cluster 3: empty
    cl[11] = 8       # cluster 8: one member (7: empty too)
    d_node, d_stat = out_buf(24 * n), out_buf(48 * k)
    d_a, d_cl = up(a), up(cl)
    ctx.cluster_stats_matrix_dev(d_a.data_ptr(), n, d_cl.data_ptr(), k, d_node.data_ptr(), d_stat.data_ptr())
    nodes, stats = st.stats_model(a, cl, k)
    assert host(d_node, 24 * n, st.NODE_DTYPE).tobytes() == nodes.tobytes()
    assert host(d_stat, 48 * k, st.CLUSTER_DTYPE).tobytes() == stats.tobytes()
    assert stats["size"][3] == 0 and stats["size"][8] == 1 and stats["size"].sum() == n


def run_nj_matrix(hg, ctx):
    """70 items, NaN on and below the diagonal (the mirror), clustered values: the n - 1 joins of the model, byte for byte; the
    last join has no update behind it, every other one has"""
    a = linkage_matrix(8)
    n = a.shape[0]
    want = nj.as_records(nj.nj_model_np(nj.dist_matrix(a)))
    joins = out_buf(24 * (n - 1))
    d_a = up(nan_below(a))
    count = ctx.nj_matrix_dev(d_a.data_ptr(), n, joins.data_ptr())
    assert count == n - 1 == want.size
    assert host(joins, 24 * (n - 1), nj.JOIN_DTYPE).tobytes() == want.tobytes()


RUNNERS = {"cluster_init_dev": run_single_linkage, "cluster_add_hits_dev": run_single_linkage, "cluster_finish_dev": run_single_linkage,
           "cluster_greedy_hits_dev": run_greedy_hits, "cluster_greedy_dev": run_greedy_blocks, "cluster_setcover_hits_dev": run_setcover_hits,
           "cluster_tree_hits_dev": run_tree_hits, "cluster_average_matrix_dev": run_average_matrix,
           "cluster_complete_matrix_dev": run_complete_matrix, "cluster_stats_matrix_dev": run_stats_matrix, "nj_matrix_dev": run_nj_matrix}


def test_every_entry_has_a_runner():
    assert {r.entry for r in cc.ROWS} == set(RUNNERS)


@pytest.mark.parametrize("row", cc.ROWS, ids=[r.name for r in cc.ROWS])
def test_census_row(hg, ctx, row):
    assert row.unreachable is None
    RUNNERS[row.entry](hg, ctx)
