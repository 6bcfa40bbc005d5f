"""hg_tri_dev, hg_tri_stream_dev and hg_tri (libhypergen_tri.so) on resident sketches: 3, 40 and 2 T + 3 of the bench's clustered
hypervectors at D = 4096 (T the columns of the kernel's tile).  Every byte `==` tests/tri_ref.py of the product's own
hg_dist_full_dev matrix of the same sketches under the same metric, whatever the rows per block are; the blocks a sink
receives, concatenated, are that text; a sink that refuses its second block ends the call with HG_ERR_IO and leaves the ctx
usable; HG_TRI_LOWER refuses the directional metric; sets of none and of one work; and a context that interleaves the call with
hg_hist_dev and the top-k search gives what fresh contexts give: the scratch block of the matrix is shared between them."""
import os
import sys

import numpy as np
import pytest

import containment_ref as cr
import hist_ref
import tri_ref

pytestmark = pytest.mark.gpu

KSIZE = 21
METRICS = (cr.MASH, cr.CONTAINMENT, cr.MAX_CONTAINMENT)
GUARD, FILL = 64, 0xA5


@pytest.fixture(scope="module")
def gctx():
    import torch
    import hypergen_amd as hg
    hg.lib_tri(), hg.lib_hist()
    with hg.Context(0) as c:
        yield c, hg, torch.device("cuda:0")


@pytest.fixture(autouse=True)
def mash_again(gctx):
    yield
    gctx[0].set_ani_metric(cr.MASH)


def full_matrix(c, hv, n2):
    import torch
    n = hv.shape[0]
    out = torch.empty(n * n, dtype=torch.float32, device=hv.device)
    torch.cuda.synchronize()
    c.dist_full_dev(hv.data_ptr(), n2.data_ptr(), n, hv.data_ptr(), n2.data_ptr(), n, hv.shape[1], KSIZE, out.data_ptr())
    c.sync()
    return out.cpu().numpy().reshape(n, n)


@pytest.fixture(scope="module")
def sets(gctx):
    """per size: the sketches on the device and, per metric, the text tri_ref makes of hg_dist_full_dev's matrix -- computed once"""
    c, hg, dev = gctx
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import bench
    T = hg.tri_geometry()["tile_cols"]
    s = {}
    for n, cluster in ((3, 2), (40, 7), (2 * T + 3, 100)):
        hv = bench.clustered_hvs(n, 0, dev, cluster=cluster)
        n2 = (hv.int() ** 2).sum(1).int()
        want = {}
        for metric in METRICS:
            c.set_ani_metric(metric)
            a = full_matrix(c, hv, n2)
            want[metric, tri_ref.FULL] = tri_ref.block_text(a, tri_ref.FULL)
            if metric != cr.CONTAINMENT:
                want[metric, tri_ref.LOWER] = tri_ref.block_text(a[:, : max(n - 1, 1)], tri_ref.LOWER)
                assert (tri_ref.milli(a) == tri_ref.milli(a.T)).all()  # (a symmetric metric: the lower triangle is the upper one's mirror)
        s[n] = (hv, n2, want)
    c.set_ani_metric(cr.MASH)
    m = tri_ref.milli(full_matrix(c, *s[40][:2]))
    assert (m == 0).sum() > 100 and (m > 90_000).sum() > 100 and len(set(m.ravel().tolist())) > 50  # unrelated pairs, clusters, many values
    return s


SIZES = ("3", "40", "2T+3")


def pick(gctx, sets, size):
    T = gctx[1].tri_geometry()["tile_cols"]
    return {"3": 3, "40": 40, "2T+3": 2 * T + 3}[size]


def tri_dev(gctx, hv, n2, layout, block_rows=0, c=None, allow=()):
    """hg_tri_dev into a text that held garbage, between two guards"""
    import torch
    ctx, hg, dev = gctx
    n = hv.shape[0]
    size = tri_ref.text_bytes(layout, 0, n, n)
    d = torch.full((GUARD + size + GUARD,), FILL, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    st = (c or ctx).tri_dev(hv.data_ptr(), n2.data_ptr(), n, hv.shape[1], KSIZE, layout, d.data_ptr() + GUARD, block_rows=block_rows, allow=allow)
    h = d.cpu().numpy()  # (final on return: no sync of the ctx)
    assert (h[:GUARD] == FILL).all() and (h[GUARD + size:] == FILL).all()
    return st, h[GUARD: GUARD + size].tobytes()


def tri_stream(gctx, hv, n2, layout, block_rows=0, c=None, refuse_at=None, allow=()):
    ctx, hg, dev = gctx
    n = hv.shape[0]
    blocks = []

    def sink(text, row0, rows):
        assert len(text) == tri_ref.text_bytes(layout, row0, rows, n)
        blocks.append((row0, rows, text))
        return 1 if refuse_at is not None and len(blocks) == refuse_at else 0

    st = (c or ctx).tri_stream_dev(hv.data_ptr(), n2.data_ptr(), n, hv.shape[1], KSIZE, layout, sink, block_rows=block_rows, allow=allow)
    return st, blocks


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("metric,layout", [(m, tri_ref.FULL) for m in METRICS] + [(cr.MASH, tri_ref.LOWER), (cr.MAX_CONTAINMENT, tri_ref.LOWER)])
def test_the_text_is_the_reference_of_the_products_own_matrix(gctx, sets, size, metric, layout):
    c, hg, dev = gctx
    n = pick(gctx, sets, size)
    hv, n2, want = sets[n]
    c.set_ani_metric(metric)
    st, got = tri_dev(gctx, hv, n2, layout)
    assert st == hg.OK and got == want[metric, layout]
    assert len(got) == 8 * (n * n if layout == tri_ref.FULL else n * (n - 1) // 2)
    if layout == tri_ref.FULL:
        assert all(got[8 * (i * n + i): 8 * (i * n + i) + 7] == b"100.000" for i in range(n))  # the diagonal as computed


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("metric,layout", [(cr.MASH, tri_ref.LOWER), (cr.CONTAINMENT, tri_ref.FULL), (cr.MAX_CONTAINMENT, tri_ref.LOWER)])
def test_the_rows_per_block_do_not_show(gctx, sets, size, metric, layout):
    c, hg, dev = gctx
    n = pick(gctx, sets, size)
    hv, n2, want = sets[n]
    c.set_ani_metric(metric)
    for block_rows in (1, 7, n):
        st, got = tri_dev(gctx, hv, n2, layout, block_rows)
        assert st == hg.OK and got == want[metric, layout], block_rows


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("metric,layout", [(cr.MASH, tri_ref.LOWER), (cr.CONTAINMENT, tri_ref.FULL), (cr.MASH, tri_ref.FULL)])
def test_the_streamed_blocks_are_the_same_text(gctx, sets, size, metric, layout):
    c, hg, dev = gctx
    n = pick(gctx, sets, size)
    hv, n2, want = sets[n]
    c.set_ani_metric(metric)
    for block_rows in (1, 7, 0):
        st, blocks = tri_stream(gctx, hv, n2, layout, block_rows)
        assert st == hg.OK
        rb = block_rows or n  # (the library's own choice holds these sets in one block)
        assert [(r0, rows) for r0, rows, _ in blocks] == [(r0, min(rb, n - r0)) for r0 in range(0, n, rb)]
        assert b"".join(t for _, _, t in blocks) == want[metric, layout]


def test_a_refusing_sink_ends_the_call_and_leaves_the_ctx_usable(gctx, sets):
    c, hg, dev = gctx
    import torch
    hv, n2, want = sets[40]
    for layout in (tri_ref.LOWER, tri_ref.FULL):
        st, blocks = tri_stream(gctx, hv, n2, layout, block_rows=7, refuse_at=2, allow=(hg.ERR_IO,))
        assert st == hg.ERR_IO and len(blocks) == 2 and "sink" in hg.lib().hg_last_error(c._h).decode()
        # the ctx afterwards: the histogram and the text are what they are
        d = torch.zeros(1001 * 8, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        assert c.hist_dev(hv.data_ptr(), n2.data_ptr(), 40, hv.data_ptr(), n2.data_ptr(), 40, hv.shape[1], KSIZE, hist_ref.UPPER, 100, d.data_ptr()) == hg.OK
        counts = d.cpu().numpy().view(np.uint64)
        assert int(counts.sum()) == 40 * 39 // 2
        fields = np.frombuffer(want[cr.MASH, tri_ref.LOWER], np.uint8).reshape(-1, 8)
        milli = np.array([int(bytes(f[:3]).strip() or b"0") * 1000 + int(bytes(f[4:7])) for f in fields])
        assert (counts == hist_ref.counts_of_milli(milli, 100)).all()
        st, got = tri_dev(gctx, hv, n2, layout, 7)
        assert st == hg.OK and got == want[cr.MASH, layout]
        st, blocks = tri_stream(gctx, hv, n2, layout, 7)
        assert st == hg.OK and b"".join(t for _, _, t in blocks) == want[cr.MASH, layout]


def test_refusals(gctx, sets):
    c, hg, dev = gctx
    hv, n2, want = sets[40]
    c.set_ani_metric(cr.CONTAINMENT)
    st, _ = tri_dev(gctx, hv, n2, tri_ref.LOWER, allow=(hg.ERR_INVALID,))
    assert st == hg.ERR_INVALID and "directional" in hg.lib().hg_last_error(c._h).decode()
    st, blocks = tri_stream(gctx, hv, n2, tri_ref.LOWER, allow=(hg.ERR_INVALID,))
    assert st == hg.ERR_INVALID and not blocks
    c.set_ani_metric(cr.MASH)
    args = (hv.data_ptr(), n2.data_ptr(), 40, hv.shape[1], KSIZE)
    import torch
    d = torch.zeros(8 * 40 * 40 + 64, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    inv = dict(allow=(hg.ERR_INVALID,))
    assert c.tri_dev(*args, 2, d.data_ptr(), **inv) == hg.ERR_INVALID                       # an unknown layout
    assert c.tri_dev(*args, tri_ref.FULL, 0, **inv) == hg.ERR_INVALID                       # no text
    assert c.tri_dev(*args, tri_ref.FULL, d.data_ptr() + 4, **inv) == hg.ERR_INVALID        # a misaligned one
    assert c.tri_dev(0, n2.data_ptr(), 40, hv.shape[1], KSIZE, tri_ref.FULL, d.data_ptr(), **inv) == hg.ERR_INVALID
    assert c.tri_dev(hv.data_ptr(), n2.data_ptr(), 40, hv.shape[1], 0, tri_ref.FULL, d.data_ptr(), **inv) == hg.ERR_INVALID
    assert c.tri_dev(hv.data_ptr(), n2.data_ptr(), 1 << 31, hv.shape[1], KSIZE, tri_ref.FULL, d.data_ptr(), allow=(hg.ERR_UNSUPPORTED,)) == hg.ERR_UNSUPPORTED
    assert not d.cpu().numpy().any()


def test_sets_of_none_and_of_one(gctx, sets):
    c, hg, dev = gctx
    hv, n2, want = sets[3]
    for layout in (tri_ref.LOWER, tri_ref.FULL):
        st, got = tri_dev(gctx, hv[:0], n2[:0], layout)
        assert st == hg.OK and got == b""
        st, blocks = tri_stream(gctx, hv[:0], n2[:0], layout)
        assert st == hg.OK and blocks == []
        st, got = tri_dev(gctx, hv[:1], n2[:1], layout)
        assert st == hg.OK and got == (b"" if layout == tri_ref.LOWER else b"100.000\n")
        st, blocks = tri_stream(gctx, hv[:1], n2[:1], layout)
        assert st == hg.OK and blocks == [(0, 1, b"" if layout == tri_ref.LOWER else b"100.000\n")]


def test_host_form(gctx, sets):
    c, hg, dev = gctx
    hv, n2, want = sets[40]
    h, hn = hv.cpu().numpy(), n2.cpu().numpy()
    assert c.tri(h, hn, hg.TRI_LOWER, KSIZE) == want[cr.MASH, tri_ref.LOWER]
    c.set_ani_metric(cr.CONTAINMENT)
    assert c.tri(h, hn, hg.TRI_FULL, KSIZE) == want[cr.CONTAINMENT, tri_ref.FULL]
    c.set_ani_metric(cr.MAX_CONTAINMENT)
    assert c.tri(h, hn, hg.TRI_LOWER, KSIZE) == want[cr.MAX_CONTAINMENT, tri_ref.LOWER]
    assert c.tri(h[:1], hn[:1], hg.TRI_LOWER, KSIZE) == b"" and c.tri(h[:0], hn[:0], hg.TRI_FULL, KSIZE) == b""


def test_one_context_shares_its_scratch_block_with_the_calls_around(gctx, sets):
    """hg_tri_dev, then hg_hist_dev, then the top-k search, then hg_tri_dev with another block height on ONE context: every result
    is what a context of its own gives"""
    import torch
    _, hg, dev = gctx
    n = pick(gctx, sets, "2T+3")
    hv, n2, want = sets[n]

    def tri_a(c):
        return tri_dev(gctx, hv, n2, tri_ref.LOWER, block_rows=150, c=c)[1]

    def hist(c):
        d = torch.full((1001 * 8,), 0xEE, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        assert c.hist_dev(hv.data_ptr(), n2.data_ptr(), n, hv.data_ptr(), n2.data_ptr(), n, hv.shape[1], KSIZE, hist_ref.UPPER, 100, d.data_ptr(),
                          block_rows=99) == hg.OK
        return d.cpu().numpy().tobytes()

    def topk(c):
        out = torch.zeros(n * 3 * 12, dtype=torch.uint8, device=dev)
        cnt = torch.zeros(n, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        c.set_debug("search_block_rows", 64)
        c.search_topk_dev(hv.data_ptr(), n2.data_ptr(), n, hv.data_ptr(), n2.data_ptr(), n, hv.shape[1], KSIZE, 85.0, 3, out.data_ptr(), cnt.data_ptr())
        c.sync()
        c.set_debug("search_block_rows", 0)
        return out.cpu().numpy().tobytes() + cnt.cpu().numpy().tobytes()

    def tri_b(c):
        return tri_dev(gctx, hv, n2, tri_ref.FULL, block_rows=33, c=c)[1]

    steps = (tri_a, hist, topk, tri_b)
    fresh = []
    for fn in steps:
        with hg.Context(0) as c:
            fresh.append(fn(c))
    with hg.Context(0) as c:
        shared = [fn(c) for fn in steps]
        again = tri_a(c)
    assert shared == fresh and again == fresh[0]
    assert fresh[0] == want[cr.MASH, tri_ref.LOWER] and fresh[3] == want[cr.MASH, tri_ref.FULL]
    assert np.frombuffer(fresh[1], np.uint64).sum() == n * (n - 1) // 2
