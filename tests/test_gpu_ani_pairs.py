"""hg_ani_pairs{,_dev}: the ANI of listed pairs, through the C ABI.  Every float is compared by its bit pattern and every dot
with ==, against tests/ani_pairs_ref.py (tests/containment_ref.py with the column layout) and against what the matrix and hit
list entry points give for the same pairs.  There is no tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest
import torch

import ani_pairs_ref as ap
import containment_ref as cr

pytestmark = pytest.mark.gpu
K = 21


@pytest.fixture(scope="module")
def hg():
    import hypergen_amd
    return hypergen_amd


@pytest.fixture(scope="module")
def ctx(hg):
    c = hg.Context(0)
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    yield c
    c.close()


@pytest.fixture
def clean_ctx(ctx):
    """the module's ctx, back on the default metric and path after each test"""
    yield ctx
    ctx.set_ani_metric(cr.MASH)
    ctx.set_debug("dist_path", "")
    ctx.enable_timing(False)


def hit_list(ij):
    import hypergen_amd as hg
    ij = np.asarray(ij, np.int64).reshape(-1, 2)
    p = np.zeros(ij.shape[0], hg.ANI_HIT_DTYPE)
    p["ref_idx"], p["qry_idx"] = ij[:, 0], ij[:, 1]
    p["ani"] = np.float32(-7.0)  # (ignored by the call)
    return p


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda()


class Sets:
    """two HV sets on the device (or one on both sides)"""

    def __init__(self, r, rn, q=None, qn=None):
        self.r, self.rn = np.ascontiguousarray(r, np.int16), np.ascontiguousarray(rn, np.int32)
        self.same = q is None
        self.q, self.qn = (self.r, self.rn) if self.same else (np.ascontiguousarray(q, np.int16), np.ascontiguousarray(qn, np.int32))
        self.d_r, self.d_rn = dev(self.r), dev(self.rn)
        self.d_q, self.d_qn = (self.d_r, self.d_rn) if self.same else (dev(self.q), dev(self.qn))
        self.R, self.Q, self.D = self.r.shape[0], self.q.shape[0], self.r.shape[1]


def run_dev(ctx, s, pairs, columns, want_dot=True, k=K):
    """hg_ani_pairs_dev on a host list: (n x popcount(columns) float32, dots or None)"""
    n, nc = pairs.size, bin(columns).count("1")
    d_pairs = dev(pairs) if n else None
    d_ani = torch.zeros(max(n * nc, 1), dtype=torch.float32, device="cuda:0")
    d_dot = torch.zeros(max(n, 1), dtype=torch.int32, device="cuda:0")
    ctx.ani_pairs_dev(s.d_r.data_ptr(), s.d_rn.data_ptr(), s.R, s.d_q.data_ptr(), s.d_qn.data_ptr(), s.Q, s.D, k,
                      d_pairs.data_ptr() if n else None, n, columns, d_ani.data_ptr() if nc else None, d_dot.data_ptr() if want_dot else None)
    return d_ani.cpu().numpy()[: n * nc].reshape(n, nc), (d_dot.cpu().numpy()[:n] if want_dot else None)


def want_for(orc, s, dots, pairs, mask=ap.ALL, k=K):
    """(reference columns, reference dots) of a list, from the exact R x Q dot matrix"""
    i, j = pairs["ref_idx"].astype(np.int64), pairs["qry_idx"].astype(np.int64)
    d = dots[i, j]
    return ap.columns(orc, mask, d, s.rn[i], s.qn[j], k), d


# ---- 1. every pair, every column ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def case1():
    r, rn, _ = cr.fragment_hvs(48, seed=5)
    q, qn, _ = cr.fragment_hvs(48, seed=6)
    q, qn = q[:40].copy(), qn[:40].copy()
    rng = np.random.default_rng(11)

    def shuffled(R, Q):
        ij = np.stack(np.meshgrid(np.arange(R), np.arange(Q), indexing="ij"), -1).reshape(-1, 2)
        ij = ij[rng.permutation(ij.shape[0])]
        return hit_list(np.concatenate([ij, ij[rng.integers(0, ij.shape[0], 200)]]))

    return {"two": (Sets(r, rn, q, qn), cr.exact_dots(r, q), shuffled(48, 40)),
            "one": (Sets(r, rn), cr.exact_dots(r, r), shuffled(48, 48))}


@pytest.mark.parametrize("which", ["two", "one"])
def test_every_pair_every_column(clean_ctx, orc, case1, which):
    ctx = clean_ctx
    s, dots, pairs = case1[which]
    assert pairs.size == s.R * s.Q + 200
    got, got_dot = run_dev(ctx, s, pairs, ap.ALL)
    want, want_dot = want_for(orc, s, dots, pairs)
    assert (got_dot == want_dot).all()
    assert ap.bits_equal(got, want)
    i, j = pairs["ref_idx"], pairs["qry_idx"]
    for metric, bit in ap.METRIC_BIT.items():  # the matrix entry point under the corresponding ctx metric, gathered
        ctx.set_ani_metric(metric)
        assert ap.bits_equal(got[:, ap.place(ap.ALL, bit)], ctx.dist_full(s.r, s.rn, s.q, s.qn, K)[i, j]), metric
    ctx.set_ani_metric(cr.CONTAINMENT)  # ... and the exchanged call, transposed
    assert ap.bits_equal(got[:, 3], ctx.dist_full(s.q, s.qn, s.r, s.rn, K).T[i, j])
    if which == "one":
        diag = (i == j) & (s.rn[i] > 0)
        assert diag.sum() >= 48 and (got[diag] == np.float32(100.0)).all()


# ---- 2. row length edges -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hv_d", [8, 56, 504, 512, 520, 4096, 4104, 8192, 65536, 1, 7, 100, 4097])
def test_row_length_edges(clean_ctx, hg, orc, hv_d):
    """6 x 5 rows whose last row ends at the last byte of its allocation; the last element of every row is large, so a dot
    that left it out -- or took in what lies behind it -- is wrong"""
    ctx = clean_ctx
    rng = np.random.default_rng(hv_d)
    lim = 3 if hv_d == 65536 else 300
    r = rng.integers(-lim, lim + 1, (6, hv_d)).astype(np.int16)
    q = rng.integers(-lim, lim + 1, (5, hv_d)).astype(np.int16)
    r[:, -1] = [20000, -20001, 19999, 20002, -19998, 20003]
    q[:, -1] = [20004, 19997, -20005, 20006, 19996]
    rn, qn = cr.norms(r), cr.norms(q)
    L = hg.lib()
    blocks = []
    try:
        for a in (r, q):
            p = C.c_void_p()
            assert L.hg_dev_alloc(ctx._h, a.nbytes, C.byref(p)) == hg.OK  # exactly the rows: the last one ends the allocation
            blocks.append(p)
            assert L.hg_copy_h2d(ctx._h, p, C.c_void_p(a.ctypes.data), a.nbytes) == hg.OK
        pairs = hit_list([(i, j) for i in range(6) for j in range(5)])
        d_rn, d_qn, d_pairs = dev(rn), dev(qn), dev(pairs)
        d_ani = torch.zeros(30 * 4, dtype=torch.float32, device="cuda:0")
        d_dot = torch.zeros(30, dtype=torch.int32, device="cuda:0")
        ctx.ani_pairs_dev(blocks[0].value, d_rn.data_ptr(), 6, blocks[1].value, d_qn.data_ptr(), 5, hv_d, K, d_pairs.data_ptr(), 30,
                          ap.ALL, d_ani.data_ptr(), d_dot.data_ptr())
        dots = cr.exact_dots(r, q).ravel()
        assert (d_dot.cpu().numpy() == dots).all()
        assert ap.bits_equal(d_ani.cpu().numpy().reshape(30, 4), ap.columns(orc, ap.ALL, dots, np.repeat(rn, 5), np.tile(qn, 6), K))
    finally:
        for p in blocks:
            L.hg_dev_free(ctx._h, p)


# ---- 3. wrapping ---------------------------------------------------------------------------------------------------------
def test_wrapping_dots_and_norms(clean_ctx, orc):
    D = 4096
    e = np.arange(D)
    rows = np.stack([np.full(D, 32767), np.full(D, -32768), np.where(e % 2 == 0, 32767, -32767), np.where(e % 2 == 0, -32768, 32767),
                     np.zeros(D, np.int64), np.where(e % 3 == 0, 32767, -32768), np.where(e < 5, 32767, 0),
                     np.where(e < 2100, -32768, 1)]).astype(np.int16)
    exact = rows.astype(np.int64) @ rows.astype(np.int64).T
    assert (np.abs(exact) > 1 << 31).sum() >= 20 and ((rows.astype(np.int64) ** 2).sum(1) > 1 << 31).sum() >= 5
    s = Sets(rows, cr.norms(rows))
    pairs = hit_list([(i, j) for i in range(8) for j in range(8)])
    got, got_dot = run_dev(clean_ctx, s, pairs, ap.ALL)
    want, want_dot = want_for(orc, s, cr.exact_dots(rows, rows), pairs)
    assert (got_dot == want_dot).all()
    assert ap.bits_equal(got, want)
    # the branches of the formula are all there: negative denominators and NaN -> 0, > 1 -> 100, values in between
    assert (want == 0).any() and (want == 100).any() and ((want > 0) & (want < 100)).any()
    assert (s.rn < 0).any() and (want_dot[pairs["ref_idx"] == 4] == 0).all() and s.rn[4] == 0


# ---- 4. list length edges -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def case4(orc):
    hv, n2, _ = cr.fragment_hvs(300, D=512, seed=9)
    s = Sets(hv, n2)
    rng = np.random.default_rng(4)
    pairs = hit_list(rng.integers(0, 300, (70001, 2)))
    want, want_dot = want_for(orc, s, cr.exact_dots(hv, hv), pairs)
    return s, pairs, want, want_dot


@pytest.mark.parametrize("n", [0, 1, 3, 4, 5, 63, 64, 65, 257, 70001])
def test_list_length_edges(clean_ctx, case4, n):
    s, pairs, want, want_dot = case4
    G, guard = 16, 0x5A5AA5A5
    d_pairs = dev(pairs[: max(n, 1)])
    buf_a = torch.full((G + n * 4 + G,), guard, dtype=torch.int32, device="cuda:0")
    buf_d = torch.full((G + n + G,), guard, dtype=torch.int32, device="cuda:0")
    clean_ctx.ani_pairs_dev(s.d_r.data_ptr(), s.d_rn.data_ptr(), s.R, s.d_q.data_ptr(), s.d_qn.data_ptr(), s.Q, s.D, K,
                            d_pairs.data_ptr(), n, ap.ALL, buf_a.data_ptr() + 4 * G, buf_d.data_ptr() + 4 * G)
    a, d = buf_a.cpu().numpy(), buf_d.cpu().numpy()
    for b in (a, d):  # nothing in front of the outputs, nothing behind them (n = 0: nothing at all)
        assert (b[:G] == guard).all() and (b[-G:] == guard).all()
    assert (d[G: G + n] == want_dot[:n]).all()
    assert (a[G: G + 4 * n].view(np.uint32) == want[:n].view(np.uint32).ravel()).all()


# ---- 5. column masks ---------------------------------------------------------------------------------------------------------
def test_column_masks(clean_ctx, hg, case4):
    ctx = clean_ctx
    s, pairs, want, want_dot = case4
    pairs, want, want_dot = pairs[:500], want[:500], want_dot[:500]
    full, _ = run_dev(ctx, s, pairs, ap.ALL)
    assert ap.bits_equal(full, want)
    for mask in range(1, 16):
        got, dot = run_dev(ctx, s, pairs, mask, want_dot=bool(mask & 1))
        assert got.shape == (500, bin(mask).count("1"))
        assert ap.bits_equal(got, full[:, [c for c, b in enumerate(ap.BITS) if mask & b]]), mask
        assert dot is None or (dot == want_dot).all()
    got, dot = run_dev(ctx, s, pairs, 0)
    assert got.shape == (500, 0) and (dot == want_dot).all()
    for mask, with_dot in ((0, False), (16, True), (16, False), (31, True)):
        with pytest.raises(hg.HgError) as e:
            run_dev(ctx, s, pairs, mask, want_dot=with_dot)
        assert e.value.status == hg.ERR_INVALID
    ctx.set_ani_metric(cr.CONTAINMENT)  # the ctx metric does not reach the call
    again, _ = run_dev(ctx, s, pairs, ap.ALL)
    assert ap.bits_equal(again, full)


# ---- 6. empty slots and bad indices --------------------------------------------------------------------------------------------
def test_empty_slots_and_bad_indices(clean_ctx, hg, orc, case1):
    ctx = clean_ctx
    s, dots, pairs = case1["two"]
    pairs = pairs[:400].copy()
    empty = np.zeros(400, bool)
    empty[[0, 5, 6, 7, 100, 399]] = True
    pairs["ref_idx"][empty] = ap.EMPTY
    pairs["qry_idx"][[0, 5]] = ap.EMPTY  # (the top-k layout's slot; an empty slot with a real qry_idx is one too)
    real = pairs[~empty]
    got, got_dot = run_dev(ctx, s, pairs, ap.ALL)
    want, want_dot = want_for(orc, s, dots, real)
    assert (got[empty].view(np.uint32) == 0).all() and (got_dot[empty] == 0).all()
    assert ap.bits_equal(got[~empty], want) and (got_dot[~empty] == want_dot).all()
    for field, value in (("ref_idx", s.R), ("qry_idx", s.Q), ("qry_idx", 0xFFFFFFFF), ("ref_idx", 0xFFFFFFFE)):
        for at in (0, 211, real.size - 1):
            bad = real.copy()
            bad[field][at] = value
            with pytest.raises(hg.HgError) as e:
                run_dev(ctx, s, bad, ap.ALL)
            assert e.value.status == hg.ERR_INVALID
            ok = np.delete(real, at)  # the same call without the record: clean, and exact
            got, got_dot = run_dev(ctx, s, ok, ap.ALL)
            assert ap.bits_equal(got, np.delete(want, at, 0)) and (got_dot == np.delete(want_dot, at)).all()


def test_topk_layout_goes_in_as_it_is(clean_ctx, case1):
    ctx = clean_ctx
    s, dots, _ = case1["two"]
    top, cnt = ctx.search_topk(s.r, s.rn, s.q, s.qn, K, ani_th=80.0, k=4)
    assert cnt.min() < 4 and cnt.max() == 4 and top.shape == (s.Q, 4)  # used and unused slots
    got, dot = run_dev(ctx, s, np.ascontiguousarray(top.ravel()), ap.MASH)
    used = (np.arange(4)[None, :] < cnt[:, None]).ravel()
    assert (top["ref_idx"].ravel()[~used] == ap.EMPTY).all()
    assert (got[used, 0].view(np.uint32) == top["ani"].ravel()[used].view(np.uint32)).all()
    assert (got[~used].view(np.uint32) == 0).all() and (dot[~used] == 0).all()


# ---- 7. behind hg_dist_dev ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def stress(orc):
    r, rn, q, qn = cr.stress_hvs(96, 80)
    dots = cr.exact_dots(r, q)
    th = {}
    for metric in ap.METRIC_BIT:  # the 300th largest value: 301 hits under mash; the containment metrics clamp ~2 200 pairs to 100
        v = np.sort(cr.ani_ref(orc, dots, rn[:, None], qn[None, :], K, metric).ravel())[::-1]
        th[metric] = float(v[300])
    return Sets(r, rn, q, qn), th


@pytest.mark.parametrize("path", ["f16", "i8", "cen"])
@pytest.mark.parametrize("metric", list(ap.METRIC_BIT))
def test_behind_dist_dev(clean_ctx, hg, stress, metric, path):
    ctx = clean_ctx
    s, th = stress
    ctx.set_ani_metric(metric)
    ctx.set_debug("dist_path", path)
    cap = s.R * s.Q
    d_hits = torch.zeros(cap * 3, dtype=torch.int32, device="cuda:0")
    n, st = ctx.dist_dev(s.d_r.data_ptr(), s.d_rn.data_ptr(), s.R, s.d_q.data_ptr(), s.d_qn.data_ptr(), s.Q, s.D, K, False, th[metric],
                         d_hits.data_ptr(), cap)
    assert st == hg.OK and 300 <= n <= 2500, n
    d_ani = torch.zeros(n, dtype=torch.float32, device="cuda:0")
    for ordered in (False, True):
        if ordered:
            ctx.sort_ani_hits_dev(d_hits.data_ptr(), n, s.Q)
        ctx.ani_pairs_dev(s.d_r.data_ptr(), s.d_rn.data_ptr(), s.R, s.d_q.data_ptr(), s.d_qn.data_ptr(), s.Q, s.D, K,
                          d_hits.data_ptr(), n, ap.METRIC_BIT[metric], d_ani.data_ptr())
        hits = d_hits.cpu().numpy()[: 3 * n].view(hg.ANI_HIT_DTYPE)
        assert (d_ani.cpu().numpy().view(np.uint32) == hits["ani"].view(np.uint32)).all(), ordered
    assert (np.diff(hits["ani"]) <= 0).all()  # (the sorted list: descending ANI)


# ---- 8. the host form ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["two", "one"])
def test_host_form(clean_ctx, case1, which):
    ctx = clean_ctx
    s, _, pairs = case1[which]
    want, want_dot = run_dev(ctx, s, pairs, ap.ALL)
    q, qn = (s.r, s.rn) if s.same else (s.q, s.qn)
    got, dot = ctx.ani_pairs(s.r, s.rn, q, qn, pairs, ap.ALL, ksize=K, want_dot=True)
    assert ap.bits_equal(got, want) and (dot == want_dot).all()
    ij = np.stack([pairs["ref_idx"], pairs["qry_idx"]], 1).astype(np.int64)  # the (n, 2) integer form, no dots
    got = ctx.ani_pairs(s.r, s.rn, q, qn, ij, ap.CONTAINMENT | ap.CONTAINMENT_REF, ksize=K)
    assert ap.bits_equal(got, want[:, [1, 3]])
    assert ctx.ani_pairs(s.r, s.rn, q, qn, ij[:0], ap.ALL).shape == (0, 4)


# ---- 9. the timing hook ----------------------------------------------------------------------------------------------------------
def test_timing_hook(clean_ctx, case4):
    ctx = clean_ctx
    s, pairs, want, _ = case4
    ctx.enable_timing(True)
    ctx.timings()
    got, _ = run_dev(ctx, s, pairs[:1000], ap.ALL)
    t = ctx.timings()
    assert t["dist"][1] == 1 and t["dist"][0] > 0 and t["dist_prep"][1] == 0
    assert ctx.last_kernel("dist") == "ani_pairs_kernel"
    assert ap.bits_equal(got, want[:1000])
