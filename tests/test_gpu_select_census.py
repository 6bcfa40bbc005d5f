"""Every support kernel (tests/select_census.py), run by the entry its census row names at one small input, and then the hit
sort, the top-k cut, the tree's edge order, the search selection and the global indices of the block calls at the shapes
where a border decides: every width of the radix sort's partial last digit and its 64-bit cap, the second chunk of its row
scan, hits a top-k call has to drop, negative and zero ANI values in the tree order, k = 31 / 32 / 33 around the search's
thread-count switch (k = 32: exactly 64 KiB of dynamic LDS), and offsets that end at the last index the entry points accept.

Every comparison is `==` on bytes or integers: against numpy / Python-integer models written here, tests/cluster_tree_ref.py,
tests/search_topk_ref.py on the device's own hg_dist_full_dev matrix, the exact references of test_gpu_kernel_census.py
(whose input builders are reused) and the CPU oracle.  Output buffers are Guards: pre-filled with 0x5A bytes, with slack
behind them that no kernel may touch.
"""
import numpy as np
import pytest
import torch

import ani_pairs_ref as apr
import cluster_tree_ref as tr
import containment_ref as cr
import dist_prep_model as dpm
import kernel_census as kc
import search_topk_ref as sref
import select_census as sc
import test_gpu_kernel_census as tkc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = 0x5A
SENT32 = SENT * 0x01010101
EMPTY = 0xFFFFFFFF
LIM31 = 2**31 - 1  # hg_dist_block_dev, hg_search_topk_block_dev: ref_off + R <= LIM31
LIM32 = 2**32 - 1  # hg_hamming_search_block_dev: ref_off + R <= LIM32
D = 4096
HIT = np.dtype([("ref_idx", "<u4"), ("qry_idx", "<u4"), ("ani", "<f4")])


@pytest.fixture(scope="module")
def hg():
    import hypergen_amd
    assert hypergen_amd.ANI_HIT_DTYPE == HIT
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
    """the module's ctx, back on the default paths and metric after each test"""
    yield mctx
    for key in ("dist_path", "dist_tile", "ham_path"):
        mctx.set_debug(key, "")
    mctx.set_ani_metric(cr.MASH)


class Guard:
    """`nbytes` of device memory for a kernel's output and `slack` bytes behind it that no kernel may touch, all of it
    pre-filled with SENT"""

    def __init__(self, nbytes, slack=256):
        self.n = int(nbytes)
        self.buf = torch.full((self.n + slack,), SENT, dtype=torch.uint8, device=DEV)
        self.ptr = self.buf.data_ptr()

    def host(self, dtype=np.uint8):
        h = self.buf.cpu().numpy()
        assert (h[self.n:] == SENT).all(), "bytes behind the output were written"
        return h[:self.n].copy().view(dtype)


def up(a):
    """a host array's bytes on the device"""
    return torch.from_numpy(np.ascontiguousarray(a).reshape(-1).view(np.uint8).copy()).to(DEV)


def same_records(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(got.view(np.uint32), want.view(np.uint32)):
        bad = np.flatnonzero((got.view(np.uint32).reshape(-1, 3) != want.view(np.uint32).reshape(-1, 3)).any(1))
        raise AssertionError((what, "first differing record", int(bad[0]), got.reshape(-1)[bad[0]], want.reshape(-1)[bad[0]], bad.size))


# ---- hit sort: dump_ani_file's order ------------------------------------------------------------------------------------
def bits_for(v):
    return max(1, int(v).bit_length())


def enum_keys(h, Q):
    """ref * Q + qry of every hit: Python integers for a list of a few thousand, uint64 arithmetic (exact: the largest key,
    (2^32 - 1) * Q + Q - 1, is below 2^64 for every Q <= 2^32) for the long ones"""
    assert (2**32 - 1) * Q + Q - 1 < 2**64 and int(h["qry_idx"].max()) < Q
    if h.size <= 10_000:
        return np.array([int(r) * Q + int(q) for r, q in zip(h["ref_idx"].tolist(), h["qry_idx"].tolist())], np.uint64)
    return h["ref_idx"].astype(np.uint64) * np.uint64(Q) + h["qry_idx"].astype(np.uint64)


def sort_model(h, Q):
    """stable ascending by ANI over the enumeration order, reversed"""
    assert not np.signbit(h["ani"]).any() and np.isfinite(h["ani"]).all()
    return h[np.lexsort((enum_keys(h, Q), h["ani"]))[::-1]]


def sort_on_device(ctx, h, Q):
    g = Guard(12 * h.size)
    g.buf[:12 * h.size] = up(h)
    ctx.sort_ani_hits_dev(g.ptr, h.size, Q)
    return g.host(HIT)


def hit_list(rng, n, Q, ani_values):
    """n hits: reference indices over all 32 bits up to 2^32 - 2 (a third of them small, the largest ones planted), query indices
    up to Q - 1 with Q - 1 itself planted, ANI values from a short list (long runs of ties: the enumeration key decides)"""
    h = np.zeros(n, HIT)
    h["ref_idx"] = rng.integers(0, 2**32 - 1, n, dtype=np.uint64).astype(np.uint32)
    h["ref_idx"][: n // 3] = rng.integers(0, 50, n // 3)
    h["qry_idx"] = rng.integers(0, Q, n, dtype=np.uint64).astype(np.uint32)
    h["ani"] = rng.choice(np.asarray(ani_values, np.float32), n)
    top = rng.choice(n, min(n, 8), replace=False)
    h["ref_idx"][top] = 2**32 - 2 - np.arange(top.size, dtype=np.uint32) // 2  # the largest keys: their top digit is the partial one
    h["qry_idx"][top[::2]] = Q - 1
    h["ani"][top] = np.float32(ani_values[0])
    return h


ANI_FEW = (85.0, 85.00001, 90.5, 99.999, 100.0, 0.0)
SORT_Q = (1, 3, 5, 9, 17, 33, 65, 129, 2**32)


def test_sort_widths_cover_every_last_digit():
    """the Q of the sort tests: key widths 33..40 -- a partial last digit of every width 1..8 -- and the cap of 64 bits"""
    widths = [min(64, 32 + bits_for(Q - 1)) for Q in SORT_Q]
    assert widths == [33, 34, 35, 36, 37, 38, 39, 40, 64]
    assert [w % 8 or 8 for w in widths[:8]] == [1, 2, 3, 4, 5, 6, 7, 8]


@pytest.mark.parametrize("Q", SORT_Q)
def test_sort_hits_every_last_digit_width(hg, ctx, Q):
    for n in (2, 4097):
        rng = np.random.default_rng(1000 * bits_for(Q) + n)
        h = hit_list(rng, n, Q, ANI_FEW)
        want = sort_model(h, Q)
        # (not vacuous: among hits of one ANI the enumeration key's highest possible bit is set in some and clear in others)
        if n > 2 and Q > 1:
            top = min(64, 32 + bits_for(Q - 1)) - 1
            k = enum_keys(h[h["ani"] == np.float32(ANI_FEW[0])], Q)
            assert ((k >> np.uint64(top)) & np.uint64(1)).any() and not ((k >> np.uint64(top)) & np.uint64(1)).all(), Q
        same_records(sort_on_device(ctx, h, Q), want, ("model", Q, n))
        same_records(hg.sort_ani_hits(h, Q), want, ("host", Q, n))
    same_records(ctx.sort_ani_hits_staged(h, Q), want, ("staged", Q))


@pytest.mark.parametrize("byte", [0, 1, 2, 3])
def test_sort_hits_ani_differs_in_one_byte_only(ctx, byte):
    """the ANI's bit patterns differ in one byte: that one of the four ANI passes decides, the other three see one digit"""
    n, Q = 4097, 9
    rng = np.random.default_rng(40 + byte)
    h = hit_list(rng, n, Q, (1.0,))
    digit = rng.integers(1, 0x7F if byte == 3 else 0x100, n).astype(np.uint32)  # (top byte: sign clear, exponent below 0xFF)
    base = np.uint32(0x12345678 & ~(0xFF << (8 * byte)))
    h["ani"] = (base | (digit << np.uint32(8 * byte))).view(np.float32)
    assert np.unique(h["ani"].view(np.uint32) >> np.uint32(8 * byte) & np.uint32(0xFF)).size > 100
    assert np.unique(h["ani"].view(np.uint32) & ~np.uint32(0xFF << (8 * byte))).size == 1
    same_records(sort_on_device(ctx, h, Q), sort_model(h, Q), byte)


def test_sort_hits_all_ani_equal_is_the_reverse_enumeration(ctx):
    n, Q = 4097, 17
    h = hit_list(np.random.default_rng(7), n, Q, (97.25,))
    got = sort_on_device(ctx, h, Q)
    k = enum_keys(got, Q)
    assert (k[:-1] >= k[1:]).all() and (k[:-1] > k[1:]).sum() > n // 2
    same_records(got, sort_model(h, Q), "equal ANI")


@pytest.mark.parametrize("n", [1_048_576, 1_048_577])
def test_sort_hits_256_and_257_tiles(hg, ctx, n):
    """a tile holds 4096 hits and radix_scan_kernel scans 256 tiles per trip: one trip exactly, and a second one of one tile"""
    assert (n + 4095) // 4096 == (256 if n % 2 == 0 else 257)
    Q = 33
    h = hit_list(np.random.default_rng(n), n, Q, ANI_FEW)
    want = sort_model(h, Q)
    same_records(sort_on_device(ctx, h, Q), want, n)
    if n % 2:
        same_records(ctx.sort_ani_hits_staged(h, Q), want, ("staged", n))


# ---- top-k per query ----------------------------------------------------------------------------------------------------
def topk_model(h, Q, k):
    """per query < Q its k best hits (ANI descending, ties: lower reference first) in a (Q, k) array, unused slots
    {0xFFFFFFFF, 0xFFFFFFFF, 0}, and min(count, k) per query; hits of a query index >= Q are dropped"""
    v = h[h["qry_idx"].astype(np.int64) < Q]
    out = np.zeros((Q, k), HIT)
    out["ref_idx"] = out["qry_idx"] = EMPTY
    cnt = np.zeros(Q, np.uint32)
    s = v[np.lexsort((v["ref_idx"], -v["ani"].astype(np.float64), v["qry_idx"]))]
    per_q = np.bincount(s["qry_idx"], minlength=Q)
    start = 0
    for q in range(Q):
        m = min(int(per_q[q]), k)
        out[q, :m] = s[start:start + m]
        cnt[q] = m
        start += int(per_q[q])
    return out, cnt


def run_topk(ctx, h, Q, k):
    out, cnt = Guard(12 * Q * k), Guard(4 * Q)
    d = up(h)
    ctx.topk_per_query_dev(d.data_ptr() if h.size else 0, h.size, Q, k, out.ptr, cnt.ptr)
    return out.host(HIT).reshape(Q, k), cnt.host(np.uint32)


def topk_list(rng, n, Q, ani_values, invalid):
    """distinct reference indices (the expected order is total); `invalid` hits carry query indices Q, Q + 1 and 0xFFFFFFFF,
    spread over the list"""
    h = np.zeros(n, HIT)
    h["ref_idx"] = rng.permutation(n).astype(np.uint32)
    h["qry_idx"] = rng.integers(0, Q, n)
    h["ani"] = rng.choice(np.asarray(ani_values, np.float32), n)
    at = rng.choice(n, invalid, replace=False)
    h["qry_idx"][at] = np.resize(np.array([Q, Q + 1, EMPTY], np.uint32), invalid)
    return h


@pytest.mark.parametrize("n,Q,k,invalid,values", [
    (3000, 37, 5, 300, ANI_FEW),      # every query has more than k hits; a tenth of the list is dropped
    (200, 37, 64, 30, ANI_FEW),       # k larger than every query's count
    (3000, 37, 1, 300, (96.5,)),      # k = 1, every ANI equal: the lowest reference wins
    (50, 1, 3, 12, ANI_FEW),          # Q = 1
    (4, 1, 3, 3, ANI_FEW),            # Q = 1 with one valid hit
    (6, 5, 2, 6, ANI_FEW),            # nothing but hits to drop: every slot empty, every count 0
], ids=["drop", "k-above-counts", "k1-equal-ani", "Q1", "Q1-one-hit", "all-dropped"])
def test_topk_drops_foreign_queries_and_writes_every_slot(ctx, n, Q, k, invalid, values):
    rng = np.random.default_rng(n + Q + k)
    h = topk_list(rng, n, Q, values, invalid)
    assert (h["qry_idx"] >= Q).sum() == invalid and set(h["qry_idx"][h["qry_idx"] >= Q].tolist()) == {Q, Q + 1, EMPTY}
    want, wcnt = topk_model(h, Q, k)
    got, cnt = run_topk(ctx, h, Q, k)
    assert np.array_equal(cnt, wcnt), (cnt, wcnt)
    same_records(got, want, (n, Q, k))
    per_q = np.bincount(h["qry_idx"][h["qry_idx"] < Q], minlength=Q)
    if k == 64:
        assert per_q.max() < k and (got["ref_idx"][:, -1] == EMPTY).all()
    if k == 1 and len(values) == 1:
        for q in range(Q):
            assert got[q, 0]["ref_idx"] == h["ref_idx"][h["qry_idx"] == q].min()
    if n == 3000 and k == 5:
        assert per_q.min() > k  # (the element k places behind a query's first belongs to the same query: the rank test runs)


# ---- the tree's edge order ----------------------------------------------------------------------------------------------
TREE_ANI = np.array([-3.5, -1e-20, -0.0, 0.0, 1e-30, 50.0, 99.5], np.float32)
TREE_TH = -50.0


def tree_hits(rng, n, per_node=3):
    """a connected graph on n nodes (node i hangs on a lower one) plus random edges, each ANI from TREE_ANI (many ties: the
    index passes decide), both orientations, a tenth of the records given twice -- once more with another ANI.  Every fourth
    node has no edge but the one it hangs on, with a negative or zero ANI: the tree must take it"""
    hi = np.arange(1, n, dtype=np.int64)
    lo = (rng.random(n - 1) * hi).astype(np.int64)
    m = per_node * n
    inner = np.flatnonzero(np.arange(n) % 4 != 3)
    a = np.concatenate([lo, rng.choice(inner, m)])
    b = np.concatenate([hi, rng.choice(inner, m)])
    b[-2:] = n - 1  # the highest index, whose top bit is the partial digit's
    assert (n - 1) % 4 != 3
    v = rng.choice(TREE_ANI, a.size)
    leaf = np.flatnonzero(hi % 4 == 3)
    v[leaf] = TREE_ANI[:4][(hi[leaf] // 4) % 4]
    flip = rng.random(a.size) < 0.5
    a, b = np.where(flip, b, a), np.where(flip, a, b)
    dup = rng.choice(a.size, max(1, a.size // 10), replace=False)
    a, b, v = np.concatenate([a, a[dup]]), np.concatenate([b, b[dup]]), np.concatenate([v, rng.choice(TREE_ANI, dup.size)])
    p = rng.permutation(a.size)
    h = np.zeros(a.size, HIT)
    h["ref_idx"], h["qry_idx"], h["ani"] = a[p], b[p], v[p]
    return h


def run_tree(ctx, n, h, th):
    tree, rep, cl = Guard(12 * (n - 1)), Guard(4 * n), Guard(4 * n)
    d = up(h)
    ne, nc = ctx.cluster_tree_hits_dev(n, d.data_ptr(), h.size, th, tree.ptr, n - 1, rep.ptr, cl.ptr)
    t = tree.host(HIT)
    assert (t[ne:].view(np.uint32) == SENT32).all(), "tree records behind the last edge were written"
    return t[:ne], rep.host(np.uint32), cl.host(np.uint32), nc


TREE_N = (2, 3, 5, 9, 17, 33, 65, 129, 257, 65_537)


def test_tree_sizes_cover_every_last_digit():
    bits = [bits_for(n - 1) for n in TREE_N]
    assert bits == [1, 2, 3, 4, 5, 6, 7, 8, 9, 17] and {b % 8 or 8 for b in bits} == set(range(1, 9))


@pytest.mark.parametrize("n", TREE_N)
def test_tree_edge_order_with_negative_and_zero_ani(ctx, n):
    rng = np.random.default_rng(n)
    h = tree_hits(rng, n)
    want = tr.tree_model(n, h["ref_idx"], h["qry_idx"], h["ani"], TREE_TH)
    assert want[3] == 1 and want[0].size == n - 1  # connected: the forest is a tree of n - 1 edges, all of them sorted
    if n >= 65:  # (not vacuous: negative values, zeros of both signs given and ties in every value)
        assert (want[0]["ani"] < 0).sum() > 3 and (want[0]["ani"] == 0).sum() > 3 and (want[0]["ani"] > 0).sum() > 3
        assert np.signbit(h["ani"][h["ani"] == 0]).any() and not np.signbit(h["ani"][h["ani"] == 0]).all()
    tree, rep, cl, nc = run_tree(ctx, n, h, TREE_TH)
    same_records(tree, want[0], n)
    assert not np.signbit(tree["ani"][tree["ani"] == 0]).any()  # -0.0 counts, and is reported, as +0.0
    assert nc == want[3] and np.array_equal(rep, want[1]) and np.array_equal(cl, want[2])
    # a threshold inside the values: the negative edges no longer count
    want = tr.tree_model(n, h["ref_idx"], h["qry_idx"], h["ani"], 0.0)
    tree, rep, cl, nc = run_tree(ctx, n, h, 0.0)
    same_records(tree, want[0], (n, "th 0"))
    assert nc == want[3] and np.array_equal(rep, want[1]) and np.array_equal(cl, want[2]) and (tree["ani"] >= 0).all()


# ---- search: the k best references per query ----------------------------------------------------------------------------
_SEARCH = {}


def search_set():
    """300 reference and 65 query sketches of graded similarity on the device; every 9th query is a copy of a reference row
    (ANI exactly 100), and rows 100..119 of the references are copies of row 7 (ties the reference index breaks)"""
    if not _SEARCH:
        hv, _, _ = cr.fragment_hvs(365, D, seed=31)
        r, q = hv[:300].copy(), hv[300:].copy()
        r[100:120] = r[7]
        q[::9] = r[(np.arange(0, 65, 9) * 13) % 300]
        r[299] = q[1]  # the last reference is some query's best
        r[5] = 0       # ANI exactly 0 with every query: counts at threshold 0, and its key is not the empty slot's
        _SEARCH.update(r=up(r).view(torch.int16), rn=up(cr.norms(r)).view(torch.int32), q=up(q).view(torch.int16),
                       qn=up(cr.norms(q)).view(torch.int32))
    return _SEARCH


def device_matrix(ctx, s, R, Q):
    out = Guard(4 * R * Q)
    ctx.dist_full_dev(s["r"].data_ptr(), s["rn"].data_ptr(), R, s["q"].data_ptr(), s["qn"].data_ptr(), Q, D, 21, out.ptr)
    return out.host(np.float32).reshape(R, Q)


def run_search(ctx, s, R, Q, th, k, ref_off=0, qry_off=0):
    out, cnt = Guard(12 * Q * k), Guard(4 * Q)
    ctx.search_topk_dev(s["r"].data_ptr(), s["rn"].data_ptr(), R, s["q"].data_ptr(), s["qn"].data_ptr(), Q, D, 21, th, k, out.ptr, cnt.ptr,
                        ref_off=ref_off, qry_off=qry_off)
    return out.host(HIT).reshape(Q, k), cnt.host(np.uint32)


def same_search(got, want, what):
    assert np.array_equal(got[1], want[1]), (what, got[1], want[1])
    same_records(got[0], want[0], what)


@pytest.mark.parametrize("Q", [1, 64, 65])
def test_search_k_31_32_33(ctx, Q):
    """plan_search: 256 threads up to k = 32 (k = 32: 64 KiB of dynamic LDS exactly), 128 from k = 33 on; one strip of 1 or 64
    columns, and a second strip of one column"""
    s = search_set()
    R = 300
    ani = device_matrix(ctx, s, R, Q)
    assert ani.min() >= 0.0 and (ani == 100.0).sum() >= 1
    top = sref.topk_sorted(ani, 33)
    for k in (31, 32, 33):
        for th in (0.0, 60.0, 100.0):
            got = run_search(ctx, s, R, Q, th, k)
            same_search(got, sref.topk_from_sorted(top, th, k), (Q, k, th))
        assert (got[1] < k).all()  # (at 100 no query fills its list: empty slots are written)
    assert (run_search(ctx, s, R, Q, 0.0, 33)[1] == 33).all()


@pytest.mark.parametrize("R", [1, 7])
def test_search_slice_shorter_than_one_trip(ctx, R):
    """Q = 1: 256 (k > 32: 128) threads share one column, a trip of the row loop covers 2048 (1024) rows -- and R has 1 or 7"""
    s = search_set()
    ani = device_matrix(ctx, s, R, 1)
    assert R == 1 or ani[5, 0] == 0.0
    for k in (1, 7, 32, 33):
        for th in (0.0, 60.0):
            got = run_search(ctx, s, R, 1, th, k)
            same_search(got, sref.topk_model(ani, th, k), (R, k, th))
        # at threshold 0 every row counts, the all-zero one among them; offsets that end at the last index only relabel
        off = run_search(ctx, s, R, 1, 0.0, k, ref_off=LIM31 - R, qry_off=LIM31 - 1)
        n = min(R, k)
        assert off[1].tolist() == [n] and np.array_equal(off[0]["ref_idx"][0, :n].astype(np.int64) - (LIM31 - R), run_search(ctx, s, R, 1, 0.0, k)[0]["ref_idx"][0, :n])
        assert (off[0]["qry_idx"][0, :n] == LIM31 - 1).all() and (off[0]["ref_idx"][0, n:] == EMPTY).all()
        if R == 7 and k >= 7:
            at = off[0]["ref_idx"][0].tolist().index(LIM31 - R + 5)
            assert at < 7 and off[0]["ani"][0, at] == 0.0


@pytest.mark.parametrize("k", [5, 32, 33])
def test_search_offsets_at_the_last_index(hg, ctx, k):
    """ref_off + R = qry_off + Q = 2^31 - 1: the offset-0 result relabelled, empty slots stay empty; one more is refused"""
    s = search_set()
    R, Q = 300, 65
    for th in (0.0, 97.0):
        base = run_search(ctx, s, R, Q, th, k)
        off = run_search(ctx, s, R, Q, th, k, ref_off=LIM31 - R, qry_off=LIM31 - Q)
        assert np.array_equal(off[1], base[1])
        live = base[0]["ref_idx"] != EMPTY
        assert live.sum() == base[1].sum() and (th == 0.0 or not live.all())
        want = base[0].copy()
        want["ref_idx"][live] += np.uint32(LIM31 - R)
        want["qry_idx"][live] += np.uint32(LIM31 - Q)
        same_records(off[0], want, (k, th))
        assert int(off[0]["ref_idx"][live].max()) == LIM31 - 1 and int(off[0]["qry_idx"][live].max()) == LIM31 - 1
    for ro, qo in ((LIM31 - R + 1, 0), (0, LIM31 - Q + 1)):
        out, cnt = Guard(12 * Q * k), Guard(4 * Q)
        with pytest.raises(hg.HgError) as e:
            ctx.search_topk_dev(s["r"].data_ptr(), s["rn"].data_ptr(), R, s["q"].data_ptr(), s["qn"].data_ptr(), Q, D, 21, 0.0, k,
                                out.ptr, cnt.ptr, ref_off=ro, qry_off=qo)
        assert e.value.status == hg.ERR_UNSUPPORTED
        assert (out.host() == SENT).all() and (cnt.host() == SENT).all()


# ---- global indices at the limit: hg_dist_block_dev -----------------------------------------------------------------------
def dist_row(name):
    row, = [r for r in kc.DIST_ROWS if r.name == name and r.entry == "dist"]
    return row


DIST_FAMILIES = {
    "128x128": (dist_row(kc.mfma_name(False, False, False, False, 4)), cr.MASH),
    "256x256": (dist_row(kc.mfma_name(False, False, True, True, 4)), cr.MASH),
    "256x320": (dist_row(kc.mfma_name(False, False, True, True, 5)), cr.MASH),
    "i8": (dist_row(kc.mfma_name(False, False, True, True, 4, i8=True)), cr.MASH),
    "centred": (dist_row(kc.mfma_name(False, False, True, True, 4, cen=True)), cr.MASH),
    "containment": (dist_row(kc.mfma_name(False, False, True, True, 4, ctm=True)), cr.MAX_CONTAINMENT),
    "skinny_q": (dist_row("dist_skinny_kernel<false>"), cr.MASH),
    "skinny_r": (dist_row("dist_skinny_kernel<true>"), cr.MASH),
    "int": (dist_row("dist_int_kernel"), cr.MASH),
}


def family_pairs(fam):
    """(two sets, one set compared with itself) of test_gpu_kernel_census.py's inputs for the family's row"""
    two, = [p for p in tkc.sets("wide" if fam == "int" else "sketch") if not p.same]
    one, = [p for p in tkc.sets("wide" if fam == "int" else "sketch") if p.same]
    if fam == "skinny_q":
        return tkc.Pair(two.r, two.q[:16]), tkc.Pair(two.q[:12])
    if fam == "skinny_r":
        return tkc.Pair(two.r[:5], two.q), tkc.Pair(two.r[:5], two.q)
    return two, one


class OnDevice:
    def __init__(self, p):
        self.R, self.Q = p.r.shape[0], p.q.shape[0]
        self.r, self.rn = up(p.r), up(p.rn)
        self.q, self.qn = (self.r, self.rn) if p.same else (up(p.q), up(p.qn))

    def block(self, ctx, ro, qo, sym, th):
        cap = self.R * self.Q
        g = Guard(12 * (cap + 8))
        n, st = ctx.dist_block_dev(self.r.data_ptr(), self.rn.data_ptr(), self.R, ro, self.q.data_ptr(), self.qn.data_ptr(), self.Q, qo,
                                   D, 21, sym, th, g.ptr, cap)
        rec = g.host(HIT)
        assert st == 0 and n <= cap and (rec[n:].view(np.uint32) == SENT32).all()
        return rec[:n]


def as_set(rec, ro=0, qo=0):
    """{(ref, qry): ANI bits} in Python integers, the offsets taken off; no pair twice"""
    out = {(int(a) - ro, int(b) - qo): int(v) for a, b, v in zip(rec["ref_idx"].tolist(), rec["qry_idx"].tolist(),
                                                                 rec["ani"].view(np.uint32).tolist())}
    assert len(out) == rec.size, "a pair was reported twice"
    return out


@pytest.mark.parametrize("fam", list(DIST_FAMILIES))
def test_dist_block_global_indices_at_the_limit(hg, ctx, orc, fam):
    row, metric = DIST_FAMILIES[fam]
    two, one = family_pairs(fam)
    for key, val in row.debug.items():
        ctx.set_debug(key, val)
    ctx.set_ani_metric(metric)
    for p, cases in ((two, ("a",)), (one, ("b", "c"))):
        dev = OnDevice(p)
        R, Q = dev.R, dev.Q
        ani = cr.ani_ref(orc, p.dots, p.rn[:, None], p.qn[None, :], 21, metric)
        for th in (tkc.thresholds(ani)[0], 0.0):
            base_rec = dev.block(ctx, 0, 0, False, th)
            assert ctx.last_kernel("dist") == row.name, (fam, ctx.last_kernel("dist"))
            tkc.assert_same_hits(base_rec, ani, th, False, (fam, th))
            base = as_set(base_rec)
            for case in cases:
                if case == "a":
                    ro, qo, sym = LIM31 - R, LIM31 - Q, False
                elif case == "b":
                    ro = qo = LIM31 - max(R, Q)
                    sym = True
                else:  # the diagonal i + ref_off == j + qry_off crosses the tiles 100 columns to the left of their own
                    shift = 100 if R > 100 else 3  # (a side of a few rows: a shift that still drops pairs)
                    ro = LIM31 - max(R, Q) - shift
                    qo, sym = ro + shift, True
                assert ro + R <= LIM31 and qo + Q <= LIM31
                got = as_set(dev.block(ctx, ro, qo, sym, th), ro, qo)
                assert ctx.last_kernel("dist") == row.name, (fam, case, ctx.last_kernel("dist"))
                want = {(i, j): v for (i, j), v in base.items() if not sym or i + ro < j + qo}
                assert got == want, (fam, case, th, len(got), len(want), sorted(set(got) ^ set(want))[:5])
                if sym:  # (not vacuous: the rule keeps pairs and -- at threshold 0 for certain -- drops pairs and meets i == j)
                    assert 0 < len(want) <= len(base)
                    assert th != 0.0 or (len(want) < len(base) and any(i + ro == j + qo for i, j in base))
    # one past the limit on either side: refused on the host, nothing written
    g = Guard(12 * 64)
    for ro, qo in ((LIM31 - dev.R + 1, 0), (0, LIM31 - dev.Q + 1)):
        with pytest.raises(hg.HgError) as e:
            ctx.dist_block_dev(dev.r.data_ptr(), dev.rn.data_ptr(), dev.R, ro, dev.q.data_ptr(), dev.qn.data_ptr(), dev.Q, qo, D, 21, False,
                               0.0, g.ptr, 64)
        assert e.value.status == hg.ERR_UNSUPPORTED
    assert (g.host() == SENT).all()


# ---- global indices at the limit: hg_hamming_search_block_dev -------------------------------------------------------------
@pytest.mark.parametrize("path", ["popc", "fp4"])
def test_hamming_block_global_indices_at_the_limit(ctx, orc, path):
    R, Q, hv_d = 300, 270, 256
    rng = np.random.default_rng(17)
    rb = rng.integers(0, 1 << 32, (R, hv_d // 32), dtype=np.uint64).astype(np.uint32)
    qb = rng.integers(0, 1 << 32, (Q, hv_d // 32), dtype=np.uint64).astype(np.uint32)
    qb[5], qb[Q - 1] = rb[R - 1], rb[0]
    want = orc.hamming_matrix(rb, qb)
    md = int(np.percentile(want, 2))
    i, j = np.nonzero(want <= md)
    exact = {(int(a), int(b)): int(want[a, b]) for a, b in zip(i, j)}
    assert 500 < len(exact) < R * Q // 10 and (R - 1, 5) in exact and (0, Q - 1) in exact
    d_r, d_q = up(rb), up(qb)
    ctx.set_debug("ham_path", path)
    for ro, qo in ((0, 0), (LIM32 - R, LIM32 - Q), (LIM32 - R, 0), (0, LIM32 - Q)):
        g = Guard(12 * (len(exact) + 8))
        n, st = ctx.hamming_search_block_dev(d_r.data_ptr(), R, ro, d_q.data_ptr(), Q, qo, hv_d, md, g.ptr, len(exact) + 8)
        assert st == 0 and n == len(exact) and ctx.last_hamming_path() == {"popc": 0, "fp4": 2}[path]
        rec = g.host(np.uint32).reshape(-1, 3)
        assert (rec[n:] == SENT32).all()
        got = {(int(a) - ro, int(b) - qo): int(c) for a, b, c in rec[:n].tolist()}
        assert len(got) == n and got == exact, (path, ro, qo)
        if ro:
            assert int(rec[:n, 0].max()) == LIM32 - 1  # the last index there is


# ---- every row at one small input ---------------------------------------------------------------------------------------
def run_prepass_row(hg, ctx, orc, row):
    """a thresholded dist call under the row's operand form on test_gpu_kernel_census.py's inputs of the class the row names:
    the path and the kernel dist_prep_model.py expects (a windowed kernel for "r512": its window length comes from
    prep_kernel's table alone) and the exact hit set.  Borders: the file select_census.py names"""
    kind = row.inputs
    p, = [p for p in tkc.sets(kind) if not p.same]
    assert p.cls == tkc.WANT_CLASS[kind]
    ctx.set_debug("dist_path", row.debug["dist_path"])
    ctx.set_debug("dist_tile", "big")
    want_path, want_name = dpm.expect_dist(p.r, p.q, row.debug["dist_path"], "big")
    assert want_path == {"f16": 0, "cen": 3, "i8": 1}[row.debug["dist_path"]]
    if row.name == "prep_kernel":
        assert dpm.raw_verdict(dpm.raw_stats(p.r), dpm.raw_stats(p.q)) == 3 and want_name == kc.mfma_name(True, False, True, True, 3)
    ani = cr.ani_ref(orc, p.dots, p.rn[:, None], p.qn[None, :], 21, cr.MASH)
    dev = OnDevice(p)
    for th in tkc.thresholds(ani)[:3]:
        rec = dev.block(ctx, 0, 0, False, th)
        assert (ctx.last_dist_path(), ctx.last_kernel("dist")) == (want_path, want_name), (row.name, ctx.last_kernel("dist"))
        tkc.assert_same_hits(rec, ani, th, False, (row.name, th))


def run_dist_ops_row(hg, ctx, orc):
    """the reference side prepared by hg_dist_prep_ops_dev, consumed by hg_dist_block_ops_dev (unpack_meta_kernel in the place of
    the reference's prepass): the exact hit set.  Borders: test_gpu_dist_ops.py"""
    p, = [p for p in tkc.sets("sketch") if not p.same]
    R, Q = p.r.shape[0], p.q.shape[0]
    L = hg.lib()
    rb, mb, Rp = L.hg_dist_ops_row_bytes(D), L.hg_dist_ops_meta_bytes(), L.hg_dist_ops_padded_rows(R)
    dev = OnDevice(p)
    ops = torch.full((Rp * rb,), SENT, dtype=torch.uint8, device=DEV)
    meta = torch.full((R * mb,), SENT, dtype=torch.uint8, device=DEV)
    flag = torch.full((1,), 77, dtype=torch.int32, device=DEV)
    ctx.set_debug("dist_path", "i8")
    ctx.dist_prep_ops_dev(dev.r.data_ptr(), R, D, ops.data_ptr(), meta.data_ptr(), flag.data_ptr())
    ctx.sync()
    assert int(flag[0]) == 0
    ani = cr.ani_ref(orc, p.dots, p.rn[:, None], p.qn[None, :], 21, cr.MASH)
    for th in tkc.thresholds(ani)[:3]:
        g = Guard(12 * (R * Q + 8))
        n, st = ctx.dist_block_ops_dev(ops.data_ptr(), meta.data_ptr(), dev.rn.data_ptr(), R, 0, 0, flag.data_ptr(), 1, dev.q.data_ptr(),
                                       dev.qn.data_ptr(), Q, 0, D, 21, False, th, g.ptr, R * Q)
        assert st == 0 and ctx.last_dist_path() == 1
        rec = g.host(HIT)
        assert (rec[n:].view(np.uint32) == SENT32).all()
        tkc.assert_same_hits(rec[:n], ani, th, False, ("dist_ops", th))


def run_pairs_row(ctx, orc):
    """every column of 500 listed pairs, one of them an empty slot: the oracle's floats and the exact dots.  Borders:
    test_gpu_ani_pairs.py"""
    p, = [p for p in tkc.sets("sketch") if not p.same]
    R, Q = p.r.shape[0], p.q.shape[0]
    rng = np.random.default_rng(5)
    pairs = np.zeros(500, HIT)
    pairs["ref_idx"], pairs["qry_idx"] = rng.integers(0, R, 500), rng.integers(0, Q, 500)
    pairs[0], pairs[1], pairs[2] = (R - 1, Q - 1, 0), (5, 0, 0), (3, 7, 0)  # last row of both, the zero rows, the duplicate
    dev = OnDevice(p)
    ani, dot = Guard(4 * 4 * 500), Guard(4 * 500)
    d_pairs = up(pairs)
    ctx.ani_pairs_dev(dev.r.data_ptr(), dev.rn.data_ptr(), R, dev.q.data_ptr(), dev.qn.data_ptr(), Q, D, 21, d_pairs.data_ptr(), 500,
                      apr.ALL, ani.ptr, dot.ptr)
    i, j = pairs["ref_idx"].astype(np.int64), pairs["qry_idx"].astype(np.int64)
    dots = p.dots[i, j]
    assert np.array_equal(dot.host(np.int32), cr.wrap_i32(dots))
    want = apr.columns(orc, apr.ALL, cr.wrap_i32(dots), p.rn[i], p.qn[j], 21)
    assert apr.bits_equal(ani.host(np.float32).reshape(500, 4), want)
    assert want[2, 0] == 100.0


def run_logf_row(ctx, orc):
    """the library's logf on 1000 floats of (0, 1] and on 1000 consecutive bit patterns.  Every float: test_gpu_ani_exact.py"""
    rng = np.random.default_rng(6)
    x = np.concatenate([rng.random(997, dtype=np.float32) + np.float32(1e-30), np.array([1.0, 0.5, 1e-38], np.float32)]).astype(np.float32)
    out, d_x = Guard(4 * x.size), up(x)
    ctx.logf_dev(out.ptr, x.size, d_x=d_x.data_ptr())
    assert np.array_equal(out.host(np.uint32), orc.logf_array(x).view(np.uint32))
    first = 0x3F000000 - 500
    out = Guard(4 * 1000)
    ctx.logf_dev(out.ptr, 1000, first_bits=first)
    want = orc.logf_array(np.arange(first, first + 1000, dtype=np.uint32).view(np.float32))
    assert np.array_equal(out.host(np.uint32), want.view(np.uint32))


def run_ani_from_dots_row(ctx, orc):
    """ANI of 1000 integer tuples (dots of the census inputs, a zero dot, a dot equal to both norms).  Borders:
    test_gpu_ani_exact.py"""
    p, = [p for p in tkc.sets("sketch") if not p.same]
    rng = np.random.default_rng(8)
    i, j = rng.integers(0, p.r.shape[0], 1000), rng.integers(0, p.q.shape[0], 1000)
    dot, nr, nq = cr.wrap_i32(p.dots[i, j]).astype(np.int32), p.rn[i].astype(np.int32), p.qn[j].astype(np.int32)
    dot[0], dot[1], nr[1], nq[1] = 0, 12345, 12345, 12345
    out, d_dot, d_nr, d_nq = Guard(4 * 1000), up(dot), up(nr), up(nq)
    for k in (1, 21, 255):
        ctx.ani_from_dots_dev(d_dot.data_ptr(), d_nr.data_ptr(), d_nq.data_ptr(), 1000, k, out.ptr)
        want = orc.ani_from_dots(dot, nr, nq, k)
        assert np.array_equal(out.host(np.uint32), np.asarray(want, np.float32).view(np.uint32)), k
    assert want[1] == 100.0 and want[0] == 0.0


def run_publish_row(ctx):
    """hg_cluster_finish_dev reads two result words back through publish_words_kernel, which clears them behind its copy: the
    cluster count of a small graph, and the count of the next call, in which the first one's must not linger"""
    n = 10
    h = np.array([(0, 1, 99.0), (1, 2, 99.0), (4, 5, 99.0), (8, 9, 99.0), (9, 8, 10.0)], HIT)
    rep, cl = Guard(4 * n), Guard(4 * n)
    d_h = up(h)
    ctx.cluster_init_dev(rep.ptr, n)
    ctx.cluster_add_hits_dev(rep.ptr, n, d_h.data_ptr(), h.size, 95.0)
    assert ctx.cluster_finish_dev(rep.ptr, n, cl.ptr) == 6
    assert rep.host(np.uint32).tolist() == [0, 0, 0, 3, 4, 4, 6, 7, 8, 8] and cl.host(np.uint32).tolist() == [0, 0, 0, 1, 2, 2, 3, 4, 5, 5]
    ctx.cluster_init_dev(rep.ptr, n)
    assert ctx.cluster_finish_dev(rep.ptr, n, cl.ptr) == n  # (the count of the call before does not linger)


@pytest.mark.parametrize("row", sc.ROWS, ids=[r.name for r in sc.ROWS])
def test_census_row(hg, ctx, orc, row):
    assert row.unreachable is None
    if row.entry == "sort_hits":
        h = hit_list(np.random.default_rng(3), 5000, 129, ANI_FEW)
        same_records(sort_on_device(ctx, h, 129), sort_model(h, 129), row.name)
    elif row.entry == "topk":
        h = topk_list(np.random.default_rng(4), 5000, 37, ANI_FEW, 100)
        want, wcnt = topk_model(h, 37, 5)
        got, cnt = run_topk(ctx, h, 37, 5)
        assert np.array_equal(cnt, wcnt)
        same_records(got, want, row.name)
    elif row.entry == "tree_edges":
        h = tree_hits(np.random.default_rng(5), 1001)
        want = tr.tree_model(1001, h["ref_idx"], h["qry_idx"], h["ani"], TREE_TH)
        tree, rep, cl, nc = run_tree(ctx, 1001, h, TREE_TH)
        same_records(tree, want[0], row.name)
        assert nc == want[3] == 1 and np.array_equal(rep, want[1]) and np.array_equal(cl, want[2])
    elif row.entry == "search":
        s = search_set()
        ani = device_matrix(ctx, s, 300, 65)
        for R in (300, 0):  # (R = 0: the emit kernel alone writes every slot empty)
            same_search(run_search(ctx, s, R, 65, 60.0, 3), sref.topk_model(ani[:R], 60.0, 3), (row.name, R))
    elif row.entry == "dist":
        run_prepass_row(hg, ctx, orc, row)
    elif row.entry == "dist_ops":
        run_dist_ops_row(hg, ctx, orc)
    elif row.entry == "pairs":
        run_pairs_row(ctx, orc)
    elif row.entry == "logf":
        run_logf_row(ctx, orc)
    elif row.entry == "ani_from_dots":
        run_ani_from_dots_row(ctx, orc)
    elif row.entry == "publish":
        run_publish_row(ctx)
    else:
        raise AssertionError(row)
