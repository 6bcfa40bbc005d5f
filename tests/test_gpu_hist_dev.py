"""hg_hist_dev and hg_hist (libhypergen_hist.so) on resident sketches: 400 of the bench's clustered hypervectors at D = 4096 against
themselves, and 37 x 211 of them for the two-set form.  Every count `==` tests/hist_ref.py of the product's own hg_dist_full_dev
matrix of the same sketches under the same metric -- and, for Mash, of the CPU oracle's matrix --, whatever the rows per block
are; the counts sum to the number of selected pairs; the selections that need one set refuse two, HG_HIST_UPPER refuses the
directional metric; and a context that ran hg_dist_dev before and hg_cluster_stats_dev behind gives what fresh contexts give:
the scratch block of the matrix is shared between them."""
import os
import sys

import numpy as np
import pytest

import containment_ref as cr
import hist_ref

pytestmark = pytest.mark.gpu

N, R2, Q2, KSIZE = 400, 37, 211, 21
METRICS = (cr.MASH, cr.CONTAINMENT, cr.MAX_CONTAINMENT)


@pytest.fixture(scope="module")
def gctx():
    import torch
    import hypergen_amd as hg
    hg.lib_hist()
    with hg.Context(0) as c:
        yield c, hg, torch.device("cuda:0")


@pytest.fixture(autouse=True)
def mash_again(gctx):
    yield
    gctx[0].set_ani_metric(cr.MASH)


def full_matrix(c, hv_r, n2_r, hv_q, n2_q):
    import torch
    out = torch.empty(hv_r.shape[0] * hv_q.shape[0], dtype=torch.float32, device=hv_r.device)
    torch.cuda.synchronize()
    c.dist_full_dev(hv_r.data_ptr(), n2_r.data_ptr(), hv_r.shape[0], hv_q.data_ptr(), n2_q.data_ptr(), hv_q.shape[0], hv_r.shape[1], KSIZE, out.data_ptr())
    c.sync()
    return out.cpu().numpy().reshape(hv_r.shape[0], hv_q.shape[0])


@pytest.fixture(scope="module")
def sets(gctx):
    """the sketches on the device and hg_dist_full_dev's matrices of them under every metric, computed once"""
    c, hg, dev = gctx
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import bench
    one = bench.clustered_hvs(N, 0, dev)
    ref, qry = bench.clustered_hvs(R2, 0, dev), bench.clustered_hvs(Q2, 0, dev, salt=1)
    norm = lambda hv: (hv.int() ** 2).sum(1).int()
    s = {"one": (one, norm(one)), "ref": (ref, norm(ref)), "qry": (qry, norm(qry)), "self": {}, "two": {}}
    for metric in METRICS:
        c.set_ani_metric(metric)
        s["self"][metric] = full_matrix(c, *s["one"], *s["one"])
        s["two"][metric] = full_matrix(c, *s["ref"], *s["qry"])
    c.set_ani_metric(cr.MASH)
    m = hist_ref.milli(s["self"][cr.MASH])
    assert (m == 0).mean() > 0.3 and (m > 90_000).sum() > N * 50  # the skew of the issue: unrelated pairs read 0, the clusters sit near the top
    return s


def hist_dev(gctx, a, b, pairs, w, block_rows=0, c=None):
    """hg_hist_dev of set a against set b (the same object: the same pointers) into a table that held garbage"""
    import torch
    ctx, hg, dev = gctx
    n = hist_ref.bins(w)
    d = torch.full((n * 8 + 64,), 0xEE, dtype=torch.uint8, device=dev)  # (hg_hist_dev zeroes the table itself)
    torch.cuda.synchronize()
    st = (c or ctx).hist_dev(a[0].data_ptr(), a[1].data_ptr(), a[0].shape[0], b[0].data_ptr(), b[1].data_ptr(), b[0].shape[0], a[0].shape[1], KSIZE,
                             pairs, w, d.data_ptr(), block_rows=block_rows)
    assert st == hg.OK
    h = d.cpu().numpy()  # (final on return: no sync of the ctx)
    assert (h[n * 8:] == 0xEE).all()
    return h[: n * 8].view(np.uint64).copy()


def same(got, want):
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "bins %s: %s != %s" % (bad[:8], got[bad[:8]], want[bad[:8]])


@pytest.mark.parametrize("metric", METRICS)
def test_every_metric_counts_its_own_matrix(gctx, sets, metric):
    c = gctx[0]
    c.set_ani_metric(metric)
    for w in (100, 1, 100_000):
        got = hist_dev(gctx, sets["one"], sets["one"], hist_ref.ALL, w)
        same(got, hist_ref.counts(sets["self"][metric], w))
        assert int(got.sum()) == N * N
        got = hist_dev(gctx, sets["ref"], sets["qry"], hist_ref.ALL, w)
        same(got, hist_ref.counts(sets["two"][metric], w))
        assert int(got.sum()) == R2 * Q2


def test_mash_counts_the_oracles_matrix(gctx, sets, orc):
    for name, (a, b) in (("self", ("one", "one")), ("two", ("ref", "qry"))):
        hv_a, n2_a, hv_b, n2_b = (t.cpu().numpy() for t in sets[a] + sets[b])
        want = np.asarray(orc.ani_matrix(hv_a, n2_a, hv_b, n2_b, KSIZE), np.float32)
        for w in (100, 1):
            same(hist_dev(gctx, sets[a], sets[b], hist_ref.ALL, w), hist_ref.counts(want, w))
        if name == "self":
            same(hist_dev(gctx, sets[a], sets[a], hist_ref.UPPER, 100), hist_ref.counts(want, 100, hist_ref.UPPER))


@pytest.mark.parametrize("block_rows", [0, 1, 7, N - 1, N])
@pytest.mark.parametrize("metric,pairs", [(cr.MASH, hist_ref.ALL), (cr.MASH, hist_ref.UPPER), (cr.MAX_CONTAINMENT, hist_ref.UPPER),
                                          (cr.CONTAINMENT, hist_ref.OFFDIAG), (cr.MASH, hist_ref.OFFDIAG)])
def test_the_rows_per_block_do_not_show(gctx, sets, metric, pairs, block_rows):
    c = gctx[0]
    c.set_ani_metric(metric)
    n_sel = {hist_ref.ALL: N * N, hist_ref.UPPER: N * (N - 1) // 2, hist_ref.OFFDIAG: N * (N - 1)}[pairs]
    for w in (100, 7):
        got = hist_dev(gctx, sets["one"], sets["one"], pairs, w, block_rows)
        same(got, hist_ref.counts(sets["self"][metric], w, pairs))
        assert int(got.sum()) == n_sel


@pytest.mark.parametrize("block_rows", [0, 1, 7, R2 - 1, R2])
def test_two_sets_in_blocks(gctx, sets, block_rows):
    c = gctx[0]
    c.set_ani_metric(cr.CONTAINMENT)
    same(hist_dev(gctx, sets["ref"], sets["qry"], hist_ref.ALL, 1, block_rows), hist_ref.counts(sets["two"][cr.CONTAINMENT], 1))


def test_host_form(gctx, sets):
    c, hg, dev = gctx
    hv, n2 = (t.cpu().numpy() for t in sets["one"])
    same(c.hist(hv, n2, pairs=hg.HIST_UPPER, bin_milli=100, ksize=KSIZE), hist_ref.counts(sets["self"][cr.MASH], 100, hist_ref.UPPER))
    rh, rn, qh, qn = (t.cpu().numpy() for t in sets["ref"] + sets["qry"])
    same(c.hist(rh, rn, qh, qn, bin_milli=1, ksize=KSIZE), hist_ref.counts(sets["two"][cr.MASH], 1))
    c.set_ani_metric(cr.CONTAINMENT)
    same(c.hist(hv, n2, pairs=hg.HIST_OFFDIAG, bin_milli=1000, ksize=KSIZE), hist_ref.counts(sets["self"][cr.CONTAINMENT], 1000, hist_ref.OFFDIAG))
    # no rows, no columns: all counts 0
    none = np.zeros((0, hv.shape[1]), np.int16), np.zeros(0, np.int32)
    assert not c.hist(*none, hv, n2, bin_milli=100).any() and not c.hist(hv, n2, *none, bin_milli=100).any()


def test_refusals(gctx, sets):
    import torch
    c, hg, dev = gctx
    (one, one_n), (ref, ref_n), (qry, qry_n) = sets["one"], sets["ref"], sets["qry"]
    d = torch.zeros(1001 * 8, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()

    def call(a, an, R, b, bn, Q, pairs, w=100, counts=None):
        return c.hist_dev(a.data_ptr(), an.data_ptr(), R, b.data_ptr(), bn.data_ptr(), Q, a.shape[1], KSIZE, pairs, w,
                          d.data_ptr() if counts is None else counts, allow=(hg.ERR_INVALID,))

    other = one.clone()
    for pairs in (hg.HIST_UPPER, hg.HIST_OFFDIAG):
        assert call(ref, ref_n, R2, qry, qry_n, Q2, pairs) == hg.ERR_INVALID       # two sets
        assert call(one, one_n, N, one, one_n, N - 1, pairs) == hg.ERR_INVALID     # the same pointers, R != Q
        assert call(one, one_n, N, other, one_n, N, pairs) == hg.ERR_INVALID       # equal rows at another address
    assert "same set" in str(hg.lib().hg_last_error(c._h).decode())
    c.set_ani_metric(cr.CONTAINMENT)
    assert call(one, one_n, N, one, one_n, N, hg.HIST_UPPER) == hg.ERR_INVALID     # directional
    assert "directional" in hg.lib().hg_last_error(c._h).decode()
    assert call(one, one_n, N, one, one_n, N, hg.HIST_OFFDIAG) == hg.OK
    c.set_ani_metric(cr.MASH)
    assert call(one, one_n, N, one, one_n, N, 3) == hg.ERR_INVALID
    assert call(one, one_n, N, one, one_n, N, hg.HIST_ALL, w=0) == hg.ERR_INVALID
    assert call(one, one_n, N, one, one_n, N, hg.HIST_ALL, w=100_001) == hg.ERR_INVALID
    assert call(one, one_n, N, one, one_n, N, hg.HIST_ALL, counts=0) == hg.ERR_INVALID


def test_one_context_shares_its_scratch_block_with_the_calls_around(gctx, sets):
    """hg_dist_dev, then hg_hist_dev, then hg_cluster_stats_dev on ONE context: every result is what a context of its own gives"""
    import torch
    _, hg, dev = gctx
    hv, n2 = sets["one"]
    cl = (torch.arange(N, device=dev) // 100).int()
    n_cl, cap = 4, N * N

    def dist(c):
        out = torch.zeros(cap * 12, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        n, st = c.dist_dev(hv.data_ptr(), n2.data_ptr(), N, hv.data_ptr(), n2.data_ptr(), N, hv.shape[1], KSIZE, True, 85.0, out.data_ptr(), cap)
        assert st == hg.OK
        hits = out.cpu().numpy()[: n * 12].view(hg.ANI_HIT_DTYPE)
        return hits[np.lexsort((hits["qry_idx"], hits["ref_idx"]))].tobytes()

    def hist(c):
        return hist_dev(gctx, sets["one"], sets["one"], hg.HIST_UPPER, 1, block_rows=150, c=c).tobytes()

    def stats(c):
        d_node = torch.zeros(N * 24, dtype=torch.uint8, device=dev)
        d_stat = torch.zeros(n_cl * 48, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        c.cluster_stats_dev(hv.data_ptr(), n2.data_ptr(), N, hv.shape[1], cl.data_ptr(), n_cl, d_node.data_ptr(), d_stat.data_ptr(), KSIZE)
        torch.cuda.synchronize()
        return d_node.cpu().numpy().tobytes() + d_stat.cpu().numpy().tobytes()

    fresh = []
    for fn in (dist, hist, stats):
        with hg.Context(0) as c:
            fresh.append(fn(c))
    with hg.Context(0) as c:
        shared = [fn(c) for fn in (dist, hist, stats)]
        again = hist(c)  # ... and behind the statistics, which left their own block in the scratch
    assert shared == fresh and again == fresh[1]
    assert len(fresh[0]) > 12 * 1000 and np.frombuffer(fresh[1], np.uint64).sum() == N * (N - 1) // 2
