"""One context, many calls: what hg_ctx carries from one call to the next ("What a context remembers") must never
show in a result.  Every section runs different entry points one after another on ONE context and compares EVERY call -- bytes,
counts, status, and where the path is predictable hg_ctx_last_dist_path / hg_ctx_last_kernel("dist") -- with the existing
reference models: containment_ref.exact_dots + ani_ref, the oracle's Hamming matrix, ani_pairs_ref, the cluster_*_ref models,
cluster_stats_ref, nj_ref, search_topk_ref and the history model of tests/ctx_history_model.py.  No tolerance anywhere.

  a. the result block w_misc / misc_zeroed across dist, Hamming, hg_ani_pairs and prepared operands: every ordered pair of
     twelve kinds of call (successes, HG_ERR_CAPACITY, vetoes, the statistics rerun, HG_ERR_INVALID, HG_ERR_INEXACT) in one
     de Bruijn walk; hg_sort_ani_hits_dev / hg_topk_per_query_dev spliced in (w_sorthits)
  b. the zero rows behind R and Q of the operand copies (i8_pad, pad_a / pad_b): a call of 1000 rows with values near each path's
     limit fills the workspaces, then R and Q shrink and grow across the tile edges, a self-comparison, a Hamming call on
     the same byte buffers, a caller's prepared operands, and the tile edge moves under the same R.  (What the section pins is
     that no result or path depends on those rows: with pad_rows returning at once it passes unchanged -- an output row of
     the GEMM depends on its own operand row alone and every prepass runs over the real rows only)
  c. path memory at R * Q = 2^24 with three contents in the same two device buffers: the i8 countdown (16 calls, 15 calls),
     the centred-path trust and rerun, metric and ksize under a trusted signature, hg_dist_full_dev in between, row blocks
  d. the slot -> tile tables: nine grids under each tile width (one more than the cache holds), the evicted and the cached one
     again, the legacy order once, one symmetric grid at five offsets
  e. the clustering result words and the shared scratch: every ordered pair of seventeen kinds of clustering call -- nine
     that succeed, each through its _dev form and its hit-list or matrix form, and eight that fail, are abandoned or are
     refused -- with the block-row hooks changing from visit to visit
  f. a seeded soak: a random sequence of all of it on one context against the same call on a fresh context
"""
import time

import numpy as np
import pytest
import torch

import ani_pairs_ref as ap
import cluster_average_ref as av
import cluster_complete_ref as cp
import cluster_greedy_ref as gr
import cluster_setcover_ref as sc
import cluster_stats_ref as st
import cluster_tree_ref as tr
import containment_ref as cr
import ctx_history_craft as H
import ctx_history_model as HM
import nj_ref as nj
import search_topk_ref as tk
import test_dist_tile_order as tile_order
import test_gpu_cluster as uf
import test_gpu_dist_boundaries as tb

pytestmark = pytest.mark.gpu
D = H.HV_D
K = 21
STRING_HOOKS = ("dist_path", "dist_tile", "dist_order", "ham_path")
NUMBER_HOOKS = ("pair_limit", "cluster_hit_cap", "average_block_rows", "complete_block_rows", "stats_block_rows", "nj_block_rows",
                "search_block_rows")


@pytest.fixture(scope="module")
def hg():
    import hypergen_amd
    hypergen_amd.lib()
    return hypergen_amd


class Session:
    """one context, its debug keys and metric as the test set them, and the history model that follows its dist calls"""

    def __init__(self, hg):
        self.hg, self.ctx, self.hist, self.hooks, self.metric, self._out = hg, hg.Context(0), HM.History(), {}, cr.MASH, None

    def debug(self, key, value):
        self.ctx.set_debug(key, str(value))
        self.hooks[key] = str(value)

    def set_metric(self, metric):
        self.ctx.set_ani_metric(metric)
        self.metric = metric

    def out(self, cap):
        if self._out is None or self._out.numel() < 3 * cap:
            self._out = torch.empty(3 * cap, dtype=torch.int32, device="cuda")
        return self._out

    def close(self):
        for key in STRING_HOOKS:
            self.ctx.set_debug(key, "")
        for key in NUMBER_HOOKS:
            self.ctx.set_debug(key, "0")
        self.ctx.set_ani_metric(cr.MASH)
        self.ctx.close()


@pytest.fixture
def session(hg):
    s = Session(hg)
    yield s
    s.close()


class Dev:
    """an i16 matrix and its norms, on the host and on the device"""

    def __init__(self, hv):
        self.h = np.ascontiguousarray(hv, np.int16)
        self.n2 = cr.norms(self.h)
        self.t, self.tn = torch.from_numpy(self.h).cuda(), torch.from_numpy(self.n2).cuda()

    def ptrs(self, first=0):
        return self.t.data_ptr() + first * self.h.shape[1] * 2, self.tn.data_ptr() + first * 4


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda()


def hits_of(hg, buf, n):
    return buf[:3 * n].cpu().numpy().view(hg.ANI_HIT_DTYPE).copy()


def assert_hits(got, ani, th, sym, ro, qo, what):
    """the hit set equals the reference matrix cut at the threshold (global indices; symmetric: ro + i < qo + j), no pair twice,
    equal ANI bits"""
    m = ani >= np.float32(th)
    if sym:
        m &= (np.arange(ani.shape[0])[:, None] + ro) < (np.arange(ani.shape[1])[None, :] + qo)
    i, j = np.nonzero(m)
    big = 1 << 32
    key = got["ref_idx"].astype(np.int64) * big + got["qry_idx"].astype(np.int64)
    want = (i.astype(np.int64) + ro) * big + j + qo
    order = np.argsort(key)
    assert np.unique(key).size == key.size, ("duplicate hits", what)
    assert key.size == want.size and (key[order] == want).all(), ("hit set", what, key.size, want.size)
    assert (got["ani"][order].view(np.uint32) == ani[i, j].view(np.uint32)).all(), ("ANI bits", what)


def threshold_for(ani, hits):
    """a value of the matrix that about `hits` entries reach"""
    flat = ani.ravel()
    return float(np.partition(flat, flat.size - hits)[flat.size - hits])


def run_dist(S, calls, ref, qry, ani, th, k=K, sym=False, ro=0, qo=0, cap=None, what=()):
    """hg_dist_block_dev on resident operands: status, count and hits against the reference, path and kernel against the history
    model.  calls: the HM.Call of the call (the debug keys and the metric are filled in here), or one per row block"""
    calls = [c._replace(dist_path=S.hooks.get("dist_path", ""), dist_tile=S.hooks.get("dist_tile", ""), metric=S.metric)
             for c in (calls if isinstance(calls, list) else [calls])]
    R, Q = sum(c.R for c in calls), calls[0].Q
    room = R * Q + 16 if cap is None else cap
    out = S.out(max(room, 1))
    torch.cuda.synchronize()  # (the context runs on its own stream)
    found, status = S.ctx.dist_block_dev(ref[0], ref[1], R, ro, qry[0], qry[1], Q, qo, calls[0].hv_d, k, sym, th, out.data_ptr(), room)
    for c in calls:
        e = S.hist.step(c)
    what = what + (calls[-1].dist_path, calls[-1].dist_tile, S.metric, k, R, Q, th, e)
    assert (S.ctx.last_dist_path(), S.ctx.last_kernel("dist")) == (e.path, e.kernel), (S.ctx.last_dist_path(), S.ctx.last_kernel("dist")) + what
    want = ani >= np.float32(th)
    if sym:
        want &= (np.arange(R)[:, None] + ro) < (np.arange(Q)[None, :] + qo)
    assert found == int(want.sum()), ("count", found, int(want.sum())) + what
    if found > room:
        assert status == S.hg.ERR_CAPACITY, what
        return None
    assert status == S.hg.OK, what
    got = hits_of(S.hg, out, found)
    assert_hits(got, ani, th, sym, ro, qo, what)
    return got


_DESCRIBED = {}


def described(tag, r, q, R, Q):
    """HM.describe of the first R and Q rows of two host matrices (q is r: one buffer), formed once per (tag, R, Q)"""
    key = (tag, R, Q, q is r)
    if key not in _DESCRIBED:
        rr = r[:R]
        _DESCRIBED[key] = HM.describe("dist", 0, 0, rr, rr if q is r and R == Q else q[:Q])
    return _DESCRIBED[key]


def call_for(tag, a, b, R=None, Q=None, entry="dist", first=0):
    """the Call of the first R rows of Dev a against the first Q of Dev b (b is a: the same buffer)"""
    R, Q = a.h.shape[0] if R is None else R, b.h.shape[0] if Q is None else Q
    return described(tag, a.h, b.h, R, Q)._replace(entry=entry, ref=a.ptrs(first)[0], qry=b.ptrs()[0])


def timed(section, t0, **counts):
    print("section %s: %.2f s; %s" % (section, time.time() - t0, ", ".join("%s = %s" % kv for kv in counts.items())))


# =========================================================================================================================
# a. the result block across families
# =========================================================================================================================
class ResultBlockCase:
    def __init__(self, hg, orc, S):
        self.hg, self.orc, self.S = hg, orc, S
        self.sets, self.ani, self.th = {}, {}, {}
        for name, (r, q) in H.a_inputs().items():
            self.sets[name] = (Dev(r), Dev(q))
            d = cr.exact_dots(r, q)
            self.ani[name] = cr.ani_ref(orc, d, cr.norms(r)[:, None], cr.norms(q)[None, :], K, cr.MASH)
            self.th[name] = threshold_for(self.ani[name], 20000)
        self.dots = cr.exact_dots(*H.a_inputs()["plain"])
        r, q = self.sets["plain"]
        self.rbits, self.qbits = orc.binarize(r.h), orc.binarize(q.h)
        self.d_rbits, self.d_qbits = up(self.rbits), up(self.qbits)
        self.ham = orc.hamming_matrix(self.rbits, self.qbits)
        self.max_dist = int(np.partition(self.ham.ravel(), 20000)[20000])
        ij = H.a_pair_list()
        self.pairs = np.zeros(ij.shape[0], hg.ANI_HIT_DTYPE)
        self.pairs["ref_idx"], self.pairs["qry_idx"] = ij[:, 0], ij[:, 1]
        self.bad_pairs = self.pairs.copy()
        self.bad_pairs["ref_idx"][250] = H.A_R  # one pair out of range
        self.want_cols = ap.columns(orc, ap.ALL, self.dots[ij[:, 0], ij[:, 1]], r.n2[ij[:, 0]], q.n2[ij[:, 1]], K)
        self.d_pairs, self.d_bad_pairs = up(self.pairs), up(self.bad_pairs)
        self.ops = {name: self.prepared(self.sets[name][0]) for name in ("plain", "i8_veto")}

    def prepared(self, dev):
        ops, meta, flag = tb.prep_ops(self.hg, self.S.ctx, dev.h)
        padded = torch.full((self.hg.lib().hg_dist_ops_padded_rows(dev.h.shape[0]), ops.shape[1]), 0x5A, dtype=torch.uint8, device="cuda")
        padded[:dev.h.shape[0]] = ops
        return padded, meta, flag

    # ---- the kinds: each makes one call and checks all of it ----
    def dist(self, name, visit, cap=None, path=""):
        S = self.S
        S.debug("dist_path", path)
        r, q = self.sets[name]
        got = run_dist(S, call_for("a-" + name, r, q), r.ptrs(), q.ptrs(), self.ani[name], self.th[name], cap=cap, what=(name, visit))
        S.debug("dist_path", "")
        return got

    def kind_dist(self, visit):
        got = self.dist("plain", visit)
        assert got.size > 0
        if visit % 2 == 0:  # the device-side orderings of the list just found (w_sorthits)
            hg, S = self.hg, self.S
            work = up(got)
            torch.cuda.synchronize()
            S.ctx.sort_ani_hits_dev(work.data_ptr(), got.size, H.A_Q)
            S.ctx.sync()
            assert np.array_equal(work.cpu().numpy().view(hg.ANI_HIT_DTYPE), hg.sort_ani_hits(got, H.A_Q)), ("sort_ani_hits_dev", visit)
            k = 3
            out = torch.empty((H.A_Q * k, 3), dtype=torch.int32, device="cuda")
            cnt = torch.empty(H.A_Q, dtype=torch.int32, device="cuda")
            src = up(got)
            torch.cuda.synchronize()
            S.ctx.topk_per_query_dev(src.data_ptr(), got.size, H.A_Q, k, out.data_ptr(), cnt.data_ptr())
            S.ctx.sync()
            top, c = out.cpu().numpy().view(hg.ANI_HIT_DTYPE).reshape(H.A_Q, k), cnt.cpu().numpy()
            per_q = np.bincount(got["qry_idx"], minlength=H.A_Q)
            assert np.array_equal(c, np.minimum(per_q, k)), ("topk counts", visit)
            s = got[np.lexsort((got["ref_idx"], -got["ani"].astype(np.float64), got["qry_idx"]))]  # qry asc, ani desc, ref asc
            starts = np.concatenate([[0], np.cumsum(per_q)[:-1]])
            for qi in range(H.A_Q):
                assert np.array_equal(top[qi, :c[qi]], s[starts[qi]:starts[qi] + c[qi]]), ("topk", visit, qi)

    def kind_dist_capacity(self, visit):
        assert self.dist("plain", visit, cap=100) is None  # (run_dist: HG_ERR_CAPACITY with the true count)

    def kind_dist_i8_veto(self, visit):
        self.dist("i8_veto", visit, path="i8")
        assert self.S.hist.log[-1][1].tried_i8 and self.S.hist.log[-1][1].path == 0

    def kind_dist_cen_veto(self, visit):
        self.dist("cen_veto", visit, path="cen")
        assert self.S.hist.log[-1][1].tried_cen and self.S.hist.log[-1][1].path == 2

    def kind_dist_rerun(self, visit):
        self.dist("rerun", visit)
        assert self.S.hist.log[-1][1].kernel.startswith("dist_mfma_kernel<true")  # the windowed kernel of the rerun

    def hamming(self, path, want_path, visit):
        S, hg = self.S, self.hg
        S.debug("ham_path", path)
        cap = H.A_R * H.A_Q
        out = S.out(cap)
        torch.cuda.synchronize()
        n, status = S.ctx.hamming_search_dev(self.d_rbits.data_ptr(), H.A_R, self.d_qbits.data_ptr(), H.A_Q, D, self.max_dist, out.data_ptr(), cap)
        S.debug("ham_path", "")
        if want_path:
            S.hist.state = HM.hamming_mfma(S.hist.state)
        what = ("hamming", path, visit)
        assert status == hg.OK and S.ctx.last_hamming_path() == want_path, what
        got = out[:3 * n].cpu().numpy().view(hg.HAM_HIT_DTYPE)
        i, j = np.nonzero(self.ham <= self.max_dist)
        key = got["ref_idx"].astype(np.int64) * H.A_Q + got["qry_idx"]
        order = np.argsort(key)
        assert n == i.size > 0 and (key[order] == i.astype(np.int64) * H.A_Q + j).all(), what + (n, i.size)
        assert (got["dist"][order] == self.ham[i, j]).all(), what

    def kind_ham_popc(self, visit):
        self.hamming("popc", 0, visit)

    def kind_ham_mfma(self, visit):
        self.hamming("mfma", 1, visit)

    def kind_ham_fp4(self, visit):
        self.hamming("fp4", 2, visit)

    def ani_pairs(self, d_pairs):
        S = self.S
        r, q = self.sets["plain"]
        n = self.pairs.size
        d_ani = torch.full((n * 4,), -3.0, dtype=torch.float32, device="cuda")
        d_dot = torch.full((n,), -3, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        S.ctx.ani_pairs_dev(r.ptrs()[0], r.ptrs()[1], H.A_R, q.ptrs()[0], q.ptrs()[1], H.A_Q, D, K, d_pairs.data_ptr(), n, ap.ALL,
                            d_ani.data_ptr(), d_dot.data_ptr())
        return d_ani.cpu().numpy().reshape(n, 4), d_dot.cpu().numpy()

    def kind_pairs(self, visit):
        cols, dots = self.ani_pairs(self.d_pairs)
        assert ap.bits_equal(cols, self.want_cols), ("ani_pairs columns", visit)
        assert (dots == self.dots[self.pairs["ref_idx"], self.pairs["qry_idx"]]).all(), ("ani_pairs dots", visit)

    def kind_pairs_invalid(self, visit):
        with pytest.raises(self.hg.HgError) as e:
            self.ani_pairs(self.d_bad_pairs)
        assert e.value.status == self.hg.ERR_INVALID, visit

    def block_ops(self, name, visit):
        S, hg = self.S, self.hg
        r, q = self.sets[name]
        ops, meta, flag = self.ops[name]
        c = call_for("a-" + name, r, q, entry="ops")._replace(dist_tile=S.hooks.get("dist_tile", ""), metric=S.metric, ref=ops.data_ptr())
        cap = H.A_R * H.A_Q + 16
        out = S.out(cap)
        torch.cuda.synchronize()
        found, status = S.ctx.dist_block_ops_dev(ops.data_ptr(), meta.data_ptr(), r.ptrs()[1], H.A_R, 0, 0, flag.data_ptr(), 1, q.ptrs()[0],
                                                 q.ptrs()[1], H.A_Q, 0, D, K, False, self.th[name], out.data_ptr(), cap)
        e = S.hist.step(c)
        what = ("block_ops", name, visit)
        if not c.i8_ok:
            assert status == hg.ERR_INEXACT and found == 0, what + (status, found)
            return
        assert status == hg.OK and (S.ctx.last_dist_path(), S.ctx.last_kernel("dist")) == (e.path, e.kernel), what + (status, S.ctx.last_kernel("dist"))
        assert_hits(hits_of(hg, out, found), self.ani[name], self.th[name], False, 0, 0, what)

    def kind_ops(self, visit):
        self.block_ops("plain", visit)

    def kind_ops_veto(self, visit):
        self.block_ops("i8_veto", visit)


def test_a_result_block_across_dist_hamming_pairs_and_prepared_operands(hg, orc, session):
    case = ResultBlockCase(hg, orc, session)
    order = H.de_bruijn_pairs(len(H.A_KINDS))
    t0 = time.time()
    for visit, kind in enumerate(order):
        getattr(case, "kind_" + H.A_KINDS[kind])(visit)
    pairs = H.pairs_of(order)
    merged = {(min(a, 10), min(b, 10)) for a, b in pairs}  # prepared operands, accepted or vetoed, as the one kind of the issue's list
    timed("a", t0, calls=len(order), ordered_pairs=len(pairs), ordered_pairs_of_eleven_kinds=len(merged))
    assert len(pairs) == 144 and len(merged) == 121


# =========================================================================================================================
# b. padding caches
# =========================================================================================================================
@pytest.mark.parametrize("path", ["i8", "cen", "f16"])
def test_b_padding_rows_behind_shrinking_and_growing_operands(hg, orc, session, path):
    S = session
    r, q = (Dev(x) for x in H.b_sets(path))
    tag = "b-" + path
    ani_rq = cr.ani_ref(orc, cr.exact_dots(r.h, q.h), r.n2[:, None], q.n2[None, :], K, cr.MASH)
    ani_rr = cr.ani_ref(orc, cr.exact_dots(r.h[:300], r.h[:300]), r.n2[:300, None], r.n2[None, :300], K, cr.MASH)
    th = threshold_for(ani_rq[:300, :333], 30000)
    hR, hQ = H.B_HAM
    rbits, qbits = orc.binarize(r.h[:hR]), orc.binarize(q.h[:hQ])
    d_rbits, d_qbits, ham = up(rbits), up(qbits), orc.hamming_matrix(rbits, qbits)
    max_dist = int(np.partition(ham.ravel(), 20000)[20000])
    ops, meta, flag = tb.prep_ops(hg, S.ctx, r.h[:300])
    padded = torch.full((hg.lib().hg_dist_ops_padded_rows(300), ops.shape[1]), 0x5A, dtype=torch.uint8, device="cuda")
    padded[:300] = ops
    want_path = {"i8": 1, "cen": 3, "f16": 0}[path]
    calls = 0
    t0 = time.time()

    def two(R, Q, what):
        run_dist(S, call_for(tag, r, q, R, Q), r.ptrs(), q.ptrs(), ani_rq[:R, :Q], th, what=(path, what))
        assert S.hist.log[-1][1].path == want_path, (path, what, R, Q)
        return 1

    S.debug("dist_path", path)
    for tile in ("big", "wide"):
        S.debug("dist_tile", tile)
        calls += two(H.B_FILL, H.B_FILL, "fill")  # rows up to 1000 of every operand copy hold values near the path's limit
        for R, Q, same in H.b_geometries():
            if same:  # one buffer on both sides: side 1 is not touched
                run_dist(S, call_for(tag, r, r, R, R), r.ptrs(), r.ptrs(), ani_rr, th, what=(path, tile, "self"))
                calls += 1
            else:
                calls += two(R, Q, tile)
        # a Hamming search on the matrix pipe reuses the byte operand buffers, then the geometry that ran before it
        S.debug("ham_path", "mfma")
        out = S.out(hR * hQ)
        torch.cuda.synchronize()
        n, status = S.ctx.hamming_search_dev(d_rbits.data_ptr(), hR, d_qbits.data_ptr(), hQ, D, max_dist, out.data_ptr(), hR * hQ)
        S.debug("ham_path", "")
        S.hist.state = HM.hamming_mfma(S.hist.state)
        got = out[:3 * n].cpu().numpy().view(hg.HAM_HIT_DTYPE)
        i, j = np.nonzero(ham <= max_dist)
        order = np.argsort(got["ref_idx"].astype(np.int64) * hQ + got["qry_idx"])
        assert status == hg.OK and S.ctx.last_hamming_path() == 1 and n == i.size and (got["ref_idx"][order] == i).all() and \
            (got["qry_idx"][order] == j).all() and (got["dist"][order] == ham[i, j]).all(), (path, tile, "hamming")
        calls += 1 + two(300, H.B_Q, "behind hamming")
        # a caller's prepared operands take side 0, then the context's own copy at the same R
        c = call_for(tag, r, q, 300, H.B_Q, entry="ops")._replace(dist_tile=tile, ref=padded.data_ptr())
        out = S.out(300 * H.B_Q + 16)
        torch.cuda.synchronize()
        found, status = S.ctx.dist_block_ops_dev(padded.data_ptr(), meta.data_ptr(), r.ptrs()[1], 300, 0, 0, flag.data_ptr(), 1, q.ptrs()[0],
                                                 q.ptrs()[1], H.B_Q, 0, D, K, False, th, out.data_ptr(), 300 * H.B_Q + 16)
        e = S.hist.step(c)
        if c.i8_ok:
            assert status == hg.OK and (S.ctx.last_dist_path(), S.ctx.last_kernel("dist")) == (e.path, e.kernel), (path, tile, "ops")
            assert_hits(hits_of(hg, out, found), ani_rq[:300, :H.B_Q], th, False, 0, 0, (path, tile, "ops"))
        else:
            assert status == hg.ERR_INEXACT and found == 0, (path, tile, "ops", status)
        assert c.i8_ok == (path == "i8")
        calls += 1 + two(300, H.B_Q, "behind ops")
    # the tile edge moves under the same R: 513 -> 300 rows at 320 columns, then 256 columns; the prepasses' statistics run
    # over whatever the rows behind R hold
    S.debug("dist_tile", "wide")
    calls += two(513, H.B_Q, "edge") + two(300, H.B_Q, "edge")
    S.debug("dist_tile", "big")
    calls += two(300, H.B_Q, "edge")
    timed("b[%s]" % path, t0, calls=calls)


# =========================================================================================================================
# c. path memory
# =========================================================================================================================
class PathMemory:
    """A, B and C in the same two device buffers; the references of each, formed once"""

    def __init__(self, hg, orc):
        self.hg, self.orc, self.S = hg, orc, Session(hg)
        r, q, rb, rc = H.pm_inputs()
        self.r, self.q = Dev(r), Dev(q)
        self.rows = {"A": r[H.PM_ROW].copy(), "B": rb, "C": rc}
        self.dots = cr.exact_dots(r, q)  # (B and C differ from A in one reference row: only that row is formed again)
        self.row_dots = {n: cr.exact_dots(row[None, :], q)[0] for n, row in self.rows.items()}
        self.row_n2 = {n: cr.norms(row[None, :]) for n, row in self.rows.items()}
        self.content = "A"
        self._ani, self._th, self.calls = {}, {}, {}
        ir, iq = HM.M.i8_rows(r), HM.M.i8_rows(q)
        for n, row in self.rows.items():
            full = H.pm_with(r, row)
            i8_ok = HM.M.i8_ok(D, ir, HM.M.i8_rows(row[None, :]), iq)  # (A's own row is accepted: the other rows' flags are A's)
            cen_ok = HM.M.cen_ok(D, HM.M.cen_rows(full), HM.M.cen_rows(q))
            self.calls[n] = HM.call("dist", self.r.ptrs()[0], self.q.ptrs()[0], H.PM_R, H.PM_Q, D, i8_ok, cen_ok, HM.M.raw_plan(full, q, True),
                                    HM.M.raw_plan(full, q, False))
        assert [(c.i8_ok, c.cen_ok) for c in self.calls.values()] == [(True, True), (False, True), (False, False)]
        rs, qs = H.small_sets()
        self.rs, self.qs = Dev(rs), Dev(qs)
        self.small_ani = cr.ani_ref(orc, cr.exact_dots(rs, qs), self.rs.n2[:, None], self.qs.n2[None, :], K, cr.MASH)
        self.small_th = threshold_for(self.small_ani, 3000)
        self.full_out = torch.empty(H.PM_R * H.PM_Q, dtype=torch.float32, device="cuda")

    def load(self, content):
        """overwrite the one row in place: pointers and sizes stay, the contents change"""
        if content != self.content:
            self.r.t[H.PM_ROW] = torch.from_numpy(self.rows[content]).cuda()
            self.r.tn[H.PM_ROW] = int(self.row_n2[content][0])
            torch.cuda.synchronize()
            self.content = content

    def ani(self, content, metric=cr.MASH, k=K):
        if (metric, k) not in self._ani:
            if len(self._ani) >= 2:  # (64 MB each: the metric sequence walks through them one after another)
                self._ani.pop(next(key for key in self._ani if key != (cr.MASH, K)))
            a = cr.ani_ref(self.orc, self.dots, self.r.n2[:, None], self.q.n2[None, :], k, metric)
            self._ani[(metric, k)] = a
            self._th[(metric, k)] = threshold_for(a, 4000)
        a = self._ani[(metric, k)]
        row = cr.ani_ref(self.orc, self.row_dots[content], self.row_n2[content], self.q.n2, k, metric)
        if not np.array_equal(a[H.PM_ROW].view(np.uint32), row.view(np.uint32)):
            a[H.PM_ROW] = row
        return a, self._th[(metric, k)]

    def big(self, content, metric=cr.MASH, k=K, calls=None):
        self.load(content)
        self.S.set_metric(metric)
        a, th = self.ani(content, metric, k)
        got = run_dist(self.S, calls or self.calls[content], self.r.ptrs(), self.q.ptrs(), a, th, k=k, cap=1 << 16, what=("c", content))
        assert 1000 < got.size < 20000
        return self.S.hist.log[-1][1]

    def small(self):
        self.S.set_metric(cr.MASH)
        run_dist(self.S, call_for("c-small", self.rs, self.qs), self.rs.ptrs(), self.qs.ptrs(), self.small_ani, self.small_th, what=("c", "small"))
        e = self.S.hist.log[-1][1]
        assert e.path == 0 and not e.tried_i8 and not e.tried_cen
        return e

    def full(self, content):
        self.load(content)
        self.S.set_metric(cr.MASH)
        a, _ = self.ani(content)
        torch.cuda.synchronize()
        self.S.ctx.dist_full_dev(self.r.ptrs()[0], self.r.ptrs()[1], H.PM_R, self.q.ptrs()[0], self.q.ptrs()[1], H.PM_Q, D, K, self.full_out.data_ptr())
        self.S.ctx.sync()
        e = self.S.hist.step(self.calls[content]._replace(entry="dist_full"))
        assert (self.S.ctx.last_dist_path(), self.S.ctx.last_kernel("dist")) == (e.path, e.kernel), (self.S.ctx.last_kernel("dist"), e)
        assert (self.full_out.cpu().numpy().view(np.uint32).reshape(a.shape) == a.view(np.uint32)).all(), "hg_dist_full_dev"


@pytest.fixture(scope="module")
def pm(hg, orc):
    p = PathMemory(hg, orc)
    yield p
    p.S.close()


@pytest.mark.parametrize("n_small", [16, 15])
def test_c_i8_countdown_after_a_trusted_veto(pm, n_small):
    """A, A, B, then n_small small unrelated calls, then A: byte operands are probed again after exactly 16 of them"""
    t0 = time.time()
    pm.small()  # (whatever the test before left: a call on other operands clears the signatures)
    while pm.S.hist.state.skip:
        pm.small()
    first, second, third = pm.big("A"), pm.big("A"), pm.big("B")
    assert (first.path, second.path, third.path, third.rerun) == (1, 1, 0, True) and pm.S.hist.state.skip == HM.SKIP_CALLS
    for _ in range(n_small):
        pm.small()
    last = pm.big("A")
    assert (last.path, last.tried_i8) == ((1, True) if n_small == 16 else (3, False)), last
    timed("c[countdown %d]" % n_small, t0, calls=4 + n_small, states=len({s for _, _, s in pm.S.hist.log}))


def test_c_centred_trust_and_rerun(pm):
    """B, B, C, B: the second B trusts the centred path, C on the trusted signature is vetoed and rerun, B starts over"""
    t0 = time.time()
    pm.small()
    while pm.S.hist.state.skip:
        pm.small()
    got = [pm.big(c) for c in ("B", "B", "C", "B")]
    assert [e.path for e in got] == [3, 3, 2, 3] and [e.rerun for e in got] == [False, False, True, False], got
    assert not any(e.tried_i8 for e in got[1:])
    timed("c[centred]", t0, calls=5)


def test_c_metric_and_ksize_under_a_trusted_signature(pm):
    t0 = time.time()
    pm.small()
    while pm.S.hist.state.skip:
        pm.small()
    assert pm.big("A").path == 1
    for metric, k in ((cr.MASH, 21), (cr.CONTAINMENT, 16), (cr.MAX_CONTAINMENT, 31), (cr.MASH, 21)):
        e = pm.big("A", metric, k)  # (trusted: no fallback behind it; the kernel and the hits are the metric's and k's)
        assert e.path == 1 and ("ctm" in e.kernel) == (metric != cr.MASH)
    pm.S.set_metric(cr.MASH)
    timed("c[metric]", t0, calls=5)


def test_c_dist_full_between_two_trusted_calls_and_row_blocks(pm):
    t0 = time.time()
    pm.small()
    while pm.S.hist.state.skip:
        pm.small()
    assert pm.big("A").path == 1
    sig = pm.S.hist.state.i8_sig
    pm.full("A")
    assert pm.S.hist.state.i8_sig == sig and pm.big("A").path == 1
    # three row blocks: the blocks' pointers and sizes are not the whole call's, and none of them is large
    limit = 2731 * H.PM_Q
    blocks = HM.blocks(H.PM_R, H.PM_Q, limit)
    assert [rows for _, rows in blocks] == [2731, 2731, 2730]
    pm.S.debug("pair_limit", limit)
    calls = [pm.calls["A"]._replace(ref=pm.r.ptrs(r0)[0], R=rows) for r0, rows in blocks]
    e = pm.big("A", calls=calls)
    pm.S.debug("pair_limit", 0)
    assert e.path == 0 and pm.S.hist.state.i8_sig is None
    assert pm.big("A").path == 1 and pm.big("A").path == 1
    timed("c[full, blocks]", t0, calls=8)


# =========================================================================================================================
# d. tile tables
# =========================================================================================================================
def test_d_tile_tables_evicted_cached_and_offset(hg, orc, session):
    S = session
    r, q = (Dev(x) for x in H.d_sets())
    ani = cr.ani_ref(orc, cr.exact_dots(r.h, q.h), r.n2[:, None], q.n2[None, :], K, cr.MASH)
    ani_rr = cr.ani_ref(orc, cr.exact_dots(r.h, r.h), r.n2[:, None], r.n2[None, :], K, cr.MASH)
    th = threshold_for(ani, 60000)
    grids = [(R, Q) for R in H.D_RS for Q in H.D_QS]
    t0 = time.time()
    calls = 0

    def one(R, Q, what):
        run_dist(S, call_for("d", r, q, R, Q), r.ptrs(), q.ptrs(), ani[:R, :Q], th, what=("d", what))
        return 1

    S.debug("dist_path", "f16")
    for tile in ("wide", "big"):
        S.debug("dist_tile", tile)
        for n, (R, Q) in enumerate(grids):  # nine tables: the first is evicted by the ninth
            if tile == "big" and n == 4:
                S.debug("dist_order", "legacy")  # no table at all, once in the middle
                calls += one(R, Q, "legacy")
                S.debug("dist_order", "")
            calls += one(R, Q, tile)
        calls += one(*grids[0], "evicted") + one(*grids[8], "cached")
    S.debug("dist_tile", "wide")
    n = H.D_RS[-1]
    for ro, qo in H.D_OFFSETS:  # one grid, the triangle moving through it; the diagonal flag both ways
        run_dist(S, call_for("d-self", r, r), r.ptrs(), r.ptrs(), ani_rr, th, sym=True, ro=ro, qo=qo, what=("d", "symmetric", ro, qo))
        calls += 1
    # the same tile counts under both widths, symmetric: only the width tells the two tables apart
    m = H.D_SYM_N
    for tile in ("big", "wide", "big"):
        S.debug("dist_tile", tile)
        run_dist(S, call_for("d-self", r, r, m, m), r.ptrs(), r.ptrs(), ani_rr[:m, :m], th, sym=True, what=("d", "symmetric", tile, m))
        calls += 1
    timed("d", t0, calls=calls, grids=2 * len(grids), offsets=len(H.D_OFFSETS))
    # host-side sanity: the order of the first and the last grid is one tests/test_dist_tile_order.py accepts
    for (R, Q), sym, ro, qo in ((grids[0], False, 0, 0), ((n, n), True, 0, 1)):
        tm, tn = (R + 255) // 256, (Q + 319) // 320
        tab = hg.dist_tile_order(tm, tn, 256, 320, False, sym, ro, qo)
        real = [(int(t) & 0xFFFF, int(t) >> 16) for t in tab[tab != tile_order.NONE]]
        assert len(real) == len(set(real)) and set(real) == tile_order.expected_tiles(tm, tn, 256, 320, sym, ro, qo)


# =========================================================================================================================
# e. clustering result words and shared scratch
# =========================================================================================================================
E_N = 150
E_KINDS = ("uf", "greedy", "setcover", "tree", "average", "complete", "stats", "nj", "search",
           "uf_bad", "greedy_bad", "setcover_bad", "tree_bad", "stats_bad", "abandon_good", "abandon_bad", "refused")
E_HOOKS = {"average_block_rows": (0, 7, 64), "complete_block_rows": (33, 0, 5), "stats_block_rows": (50, 3, 0), "nj_block_rows": (0, 11, 128),
           "search_block_rows": (13, 0, 100), "cluster_hit_cap": (0, 64, 100000), "pair_limit": (0, E_N * 20, E_N * 57)}


_E_REFERENCE = {}


def e_reference(orc):
    """the section's sketches, their ANI matrix, the two thresholds and every model's answer at each, formed once per module"""
    if _E_REFERENCE:
        return _E_REFERENCE
    import bench
    n = E_N
    hv = bench.clustered_hvs(n, 0, torch.device("cuda:0"), cluster=25)[:, :D].contiguous().cpu().numpy()
    n2 = cr.norms(hv)
    ani = cr.ani_ref(orc, cr.exact_dots(hv, hv), n2[:, None], n2[None, :], K, cr.MASH)
    within = ani[np.triu(np.arange(n)[:, None] // 25 == np.arange(n)[None, :] // 25, 1)]
    ths = (float(np.quantile(within, 0.5)), float(np.quantile(within, 0.02)))
    want = {}
    for th in ths:
        i, j = np.nonzero(np.triu(ani >= np.float32(th), 1))
        h = uf.hits_array(i, j, ani[i, j])
        bad = h.copy()
        bad["qry_idx"][len(bad) // 2] = n  # one hit with an index >= n
        rep, cl, nc = uf.model(n, i, j)
        assert 1 < nc < n and h.size > n
        bad_cl = cl.copy()
        bad_cl[n - 1] = nc  # one id >= n_clusters
        want[th] = {"hits": h, "bad": bad, "cl": cl, "bad_cl": bad_cl, "uf": (rep, cl, nc), "greedy": gr.greedy_model(n, i, j, ani[i, j], th),
                    "setcover": sc.setcover_model(n, i, j, ani[i, j], th), "tree": tr.tree_model(n, i, j, ani[i, j], th),
                    "average": av.average_model(ani, th), "complete": cp.complete_model(ani, th), "stats": st.stats_model(ani, cl, nc),
                    "search": tk.topk_model(ani, th, 5)}
    _E_REFERENCE.update(hv=hv, ani=ani, ths=ths, want=want, nj=nj.as_records(nj.nj_model_np(nj.dist_matrix(ani))))
    return _E_REFERENCE


class ClusterCase:
    def __init__(self, hg, orc, S):
        self.hg, self.S, self.c = hg, S, S.ctx
        ref = e_reference(orc)
        self.hv, self.ani, self.ths, self.nj = Dev(ref["hv"]), ref["ani"], ref["ths"], ref["nj"]
        self.d_ani = torch.from_numpy(self.ani).cuda()
        self.want = {th: dict(w, d_hits=up(w["hits"]), d_bad=up(w["bad"]), d_cl=up(w["cl"]), d_bad_cl=up(w["bad_cl"])) for th, w in ref["want"].items()}
        self.i32 = lambda fill=-1: torch.full((E_N,), fill, dtype=torch.int32, device="cuda")
        self.f32 = lambda: torch.full((E_N,), -1.0, dtype=torch.float32, device="cuda")

    def u32(self, t):
        return t.cpu().numpy().view(np.uint32)

    def fails(self, status, fn, *args):
        with pytest.raises(self.hg.HgError) as e:
            fn(*args)
        assert e.value.status == status, (e.value, status)

    # ---- the kinds that succeed: the _dev form, then the hit-list or matrix form ----
    def kind_uf(self, th, w):
        c, n, hv = self.c, E_N, self.hv
        rep, cl = self.i32(), self.i32()
        torch.cuda.synchronize()
        nc = c.cluster_dev(*hv.ptrs(), n, D, rep.data_ptr(), cl.data_ptr(), K, th)
        uf.assert_same((self.u32(rep), self.u32(cl), nc), w["uf"])
        rep, cl = self.i32(), self.i32()
        torch.cuda.synchronize()
        c.cluster_init_dev(rep.data_ptr(), n)
        half = w["hits"].size // 2
        c.cluster_add_hits_dev(rep.data_ptr(), n, w["d_hits"].data_ptr(), half, th)
        c.cluster_add_hits_dev(rep.data_ptr(), n, w["d_hits"].data_ptr() + 12 * half, w["hits"].size - half, th)
        nc = c.cluster_finish_dev(rep.data_ptr(), n, cl.data_ptr())
        uf.assert_same((self.u32(rep), self.u32(cl), nc), w["uf"])

    def rep_scheme(self, name, th, w, dev_fn, hits_fn):
        n, hv = E_N, self.hv
        for form in ("dev", "hits"):
            rep, cl, ani = self.i32(), self.i32(), self.f32()
            torch.cuda.synchronize()
            if form == "dev":
                nc = dev_fn(*hv.ptrs(), n, D, rep.data_ptr(), cl.data_ptr(), ani.data_ptr(), K, th)
            else:
                nc = hits_fn(n, w["d_hits"].data_ptr(), w["hits"].size, th, rep.data_ptr(), cl.data_ptr(), ani.data_ptr())
            want = w[name]
            assert nc == want[3] and np.array_equal(self.u32(rep), want[0]) and np.array_equal(self.u32(cl), want[1]), (name, form, th)
            assert np.array_equal(ani.cpu().numpy().view(np.uint32), want[2].view(np.uint32)), (name, form, th, "ani")

    def kind_greedy(self, th, w):
        self.rep_scheme("greedy", th, w, self.c.cluster_greedy_dev, self.c.cluster_greedy_hits_dev)

    def kind_setcover(self, th, w):
        self.rep_scheme("setcover", th, w, self.c.cluster_setcover_dev, self.c.cluster_setcover_hits_dev)

    def kind_tree(self, th, w):
        c, n, hv = self.c, E_N, self.hv
        for form in ("dev", "hits"):
            rep, cl = self.i32(), self.i32()
            tree = torch.full((3 * (n - 1),), -1, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            if form == "dev":
                ne, nc = c.cluster_tree_dev(*hv.ptrs(), n, D, tree.data_ptr(), n - 1, rep.data_ptr(), cl.data_ptr(), K, th)
            else:
                ne, nc = c.cluster_tree_hits_dev(n, w["d_hits"].data_ptr(), w["hits"].size, th, tree.data_ptr(), n - 1, rep.data_ptr(), cl.data_ptr())
            want = w["tree"]
            got = tree[:3 * ne].cpu().numpy().view(self.hg.ANI_HIT_DTYPE)
            assert nc == want[3] and got.tobytes() == want[0].tobytes(), ("tree", form, th)
            assert np.array_equal(self.u32(rep), want[1]) and np.array_equal(self.u32(cl), want[2]), ("tree", form, th)

    def linkage(self, name, th, w, dev_fn, matrix_fn):
        n, hv = E_N, self.hv
        for form in ("dev", "matrix"):
            rep, cl, into, level, size = self.i32(), self.i32(), self.i32(), self.f32(), self.i32()
            torch.cuda.synchronize()
            tail = (rep.data_ptr(), cl.data_ptr(), into.data_ptr(), level.data_ptr(), size.data_ptr())
            nc = dev_fn(*hv.ptrs(), n, D, *tail, K, th) if form == "dev" else matrix_fn(self.d_ani.data_ptr(), n, th, *tail)
            want = w[name]
            assert nc == want[5], (name, form, th, nc, want[5])
            for got, ref, what in zip((rep, cl, into, level, size), want, ("rep", "cluster", "into", "level", "size")):
                assert np.array_equal(got.cpu().numpy().view(np.uint32), ref.view(np.uint32)), (name, form, th, what)

    def kind_average(self, th, w):
        self.linkage("average", th, w, self.c.cluster_average_dev, self.c.cluster_average_matrix_dev)

    def kind_complete(self, th, w):
        self.linkage("complete", th, w, self.c.cluster_complete_dev, self.c.cluster_complete_matrix_dev)

    def kind_stats(self, th, w):
        c, n, hv = self.c, E_N, self.hv
        k = w["uf"][2]
        for form in ("dev", "matrix"):
            node = torch.full((n * 24,), 0xAB, dtype=torch.uint8, device="cuda")
            stat = torch.full((k * 48,), 0xAB, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            if form == "dev":
                c.cluster_stats_dev(*hv.ptrs(), n, D, w["d_cl"].data_ptr(), k, node.data_ptr(), stat.data_ptr(), K)
            else:
                c.cluster_stats_matrix_dev(self.d_ani.data_ptr(), n, w["d_cl"].data_ptr(), k, node.data_ptr(), stat.data_ptr())
            got = (node.cpu().numpy().view(st.NODE_DTYPE), stat.cpu().numpy().view(st.CLUSTER_DTYPE))
            for g, ref, what in zip(got, w["stats"], ("node", "cluster")):
                assert g.dtype == ref.dtype and g.shape == ref.shape, ("stats", form, th, what)
                for name in ref.dtype.names:
                    assert np.array_equal(g[name], ref[name]), ("stats", form, th, what, name)

    def kind_nj(self, th, w):
        c, n, hv = self.c, E_N, self.hv
        for form in ("dev", "matrix"):
            out = torch.full(((n - 1) * 24,), 0xA5, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            count = c.nj_dev(*hv.ptrs(), n, D, out.data_ptr(), K) if form == "dev" else c.nj_matrix_dev(self.d_ani.data_ptr(), n, out.data_ptr())
            assert count == n - 1 and out.cpu().numpy().tobytes() == self.nj.tobytes(), ("nj", form)

    def kind_search(self, th, w):
        c, n, hv = self.c, E_N, self.hv
        out = torch.full((n * 5 * 3,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        cnt = torch.full((n,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        c.search_topk_dev(*hv.ptrs(), n, *hv.ptrs(), n, D, K, th, 5, out.data_ptr(), cnt.data_ptr())
        c.sync()
        got = out.cpu().numpy().view(np.uint8).view(tk.HIT_DTYPE).reshape(n, 5)
        assert np.array_equal(cnt.cpu().numpy().view(np.uint32), w["search"][1]) and np.array_equal(got, w["search"][0]), ("search", th)

    # ---- the kinds that fail, are abandoned or are refused ----
    def incremental(self, th, d_hits, n_hits):
        rep = self.i32()
        torch.cuda.synchronize()
        self.c.cluster_init_dev(rep.data_ptr(), E_N)
        self.c.cluster_add_hits_dev(rep.data_ptr(), E_N, d_hits.data_ptr(), n_hits, th)
        return rep

    def kind_uf_bad(self, th, w):
        rep, cl = self.incremental(th, w["d_bad"], w["hits"].size), self.i32()
        self.fails(self.hg.ERR_INVALID, self.c.cluster_finish_dev, rep.data_ptr(), E_N, cl.data_ptr())

    def kind_greedy_bad(self, th, w):
        rep, cl = self.i32(), self.i32()
        self.fails(self.hg.ERR_INVALID, self.c.cluster_greedy_hits_dev, E_N, w["d_bad"].data_ptr(), w["hits"].size, th, rep.data_ptr(), cl.data_ptr())

    def kind_setcover_bad(self, th, w):
        rep, cl = self.i32(), self.i32()
        self.fails(self.hg.ERR_INVALID, self.c.cluster_setcover_hits_dev, E_N, w["d_bad"].data_ptr(), w["hits"].size, th, rep.data_ptr(), cl.data_ptr())

    def kind_tree_bad(self, th, w):
        tree = torch.full((3 * (E_N - 1),), -1, dtype=torch.int32, device="cuda")
        self.fails(self.hg.ERR_INVALID, self.c.cluster_tree_hits_dev, E_N, w["d_bad"].data_ptr(), w["hits"].size, th, tree.data_ptr(), E_N - 1)

    def kind_stats_bad(self, th, w):
        node = torch.full((E_N * 24,), 0xAB, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        self.fails(self.hg.ERR_INVALID, self.c.cluster_stats_matrix_dev, self.d_ani.data_ptr(), E_N, w["d_bad_cl"].data_ptr(), w["uf"][2], node.data_ptr())

    def kind_abandon_good(self, th, w):
        self.incremental(th, w["d_hits"], w["hits"].size)  # ... and the sequence is dropped, which is legal
        self.c.sync()

    def kind_abandon_bad(self, th, w):
        self.incremental(th, w["d_bad"], w["hits"].size)
        self.c.sync()

    def kind_refused(self, th, w):
        rep, cl = self.i32(), self.i32()
        if th == self.ths[0]:  # by the directional metric, before anything is queued
            self.S.set_metric(cr.CONTAINMENT)
            self.fails(self.hg.ERR_INVALID, self.c.cluster_dev, *self.hv.ptrs(), E_N, D, rep.data_ptr(), cl.data_ptr(), K, th)
            self.S.set_metric(cr.MASH)
        else:  # by n above the scheme's limit
            self.fails(self.hg.ERR_UNSUPPORTED, self.c.cluster_average_matrix_dev, self.d_ani.data_ptr(), self.hg.CLUSTER_AVERAGE_MAX_N + 1, th,
                       rep.data_ptr(), cl.data_ptr())


def test_e_clustering_calls_in_every_order(hg, orc, session):
    S = session
    case = ClusterCase(hg, orc, S)
    t0 = time.time()
    # set cover appends to the shared hit list: behind a call that left the list large, starting small (the grow path keeps
    # the hits of the blocks before) and at its own size
    for cap in (100000, 64, 0):
        S.debug("cluster_hit_cap", cap)
        S.debug("pair_limit", E_N * 20)
        (case.kind_uf if cap == 100000 else case.kind_setcover)(case.ths[1], case.want[case.ths[1]])
    order = H.de_bruijn_pairs(len(E_KINDS))
    for visit, kind in enumerate(order):
        for key, values in E_HOOKS.items():  # consecutive users of the shared scratch disagree about its shape
            S.debug(key, values[visit % 3])
        th = case.ths[(visit // 3) % 2]
        try:
            getattr(case, "kind_" + E_KINDS[kind])(th, case.want[th])
        except Exception:
            print("section e: visit %d, %s behind %s, threshold %r, hooks %r" % (visit, E_KINDS[kind], E_KINDS[order[visit - 1]] if visit else None, th, S.hooks))
            raise
    pairs = H.pairs_of(order)
    behind_failures = {(a, b) for a, b in pairs if a >= 9}
    timed("e", t0, visits=len(order), ordered_pairs=len(pairs), ordered_pairs_behind_a_failure=len(behind_failures))
    assert len(pairs) == 17 * 17 and len(behind_failures) == 8 * 17


def test_e_stats_behind_an_abandoned_sequence_with_a_bad_hit(hg, orc, session):
    """the one transition the inventory predicted wrong, on its own: init, add_hits with an index >= n, nothing else -- and the
    statistics of valid ids on the same context are the model's"""
    case = ClusterCase(hg, orc, session)
    th = case.ths[0]
    case.kind_abandon_bad(th, case.want[th])
    case.kind_stats(th, case.want[th])


# =========================================================================================================================
# f. a seeded soak: one context against a fresh one per call
# =========================================================================================================================
SOAK_SEED = 20240607
SOAK_CALLS = 400  # (0.26 s for 60 calls on the MI355X, fresh contexts included)


class Soak:
    """the calls, each a function of (context, parameters) that returns everything the call reports, in a canonical order"""

    def __init__(self, hg, orc):
        import bench
        self.hg = hg
        r, q = H.C.two_sets(D, 0, 1, 950, r=400, q=400)
        self.r, self.q = Dev(r), Dev(q)
        self.cl = Dev(bench.clustered_hvs(400, 0, torch.device("cuda:0"), cluster=20)[:, :D].contiguous().cpu().numpy())
        self.rbits, self.qbits = up(orc.binarize(r)), up(orc.binarize(q))
        self.th = threshold_for(cr.ani_ref(orc, cr.exact_dots(r[:100], q[:100]), self.r.n2[:100, None], self.q.n2[None, :100], K, cr.MASH), 3000)

    def params(self, rng):
        kind = ("dist", "dist", "dist_full", "hamming", "pairs", "uf", "greedy", "setcover", "tree", "average", "complete", "stats", "nj",
                "search", "abandon_bad", "stats_bad")[int(rng.integers(0, 16))]
        return {"kind": kind, "R": int(rng.integers(40, 401)), "Q": int(rng.integers(40, 401)), "first": int(rng.integers(0, 2)) * 3,
                "path": ("", "i8", "cen", "f16")[int(rng.integers(0, 4))], "tile": ("", "big", "wide", "small")[int(rng.integers(0, 4))],
                "ham": ("popc", "mfma", "fp4")[int(rng.integers(0, 3))], "metric": (cr.MASH, cr.MAX_CONTAINMENT)[int(rng.integers(0, 2))],
                "rows": int(rng.integers(0, 3)) * 17, "cap": (0, 64)[int(rng.integers(0, 2))], "sym": bool(rng.integers(0, 2))}

    def run(self, c, p):
        hg, kind, R, Q = self.hg, p["kind"], p["R"], p["Q"]
        c.set_ani_metric(p["metric"])
        for key, value in (("dist_path", p["path"]), ("dist_tile", p["tile"]), ("ham_path", p["ham"]), ("cluster_hit_cap", p["cap"])):
            c.set_debug(key, str(value))
        for key in ("average_block_rows", "complete_block_rows", "stats_block_rows", "nj_block_rows", "search_block_rows"):
            c.set_debug(key, str(p["rows"]))
        R = min(R, 400 - p["first"])
        rp, qp = self.r.ptrs(p["first"]), self.q.ptrs()
        n = min(R, 150) if kind in ("nj", "average", "complete") else R
        cp_ = self.cl.ptrs(p["first"])
        i32 = lambda m=n: torch.full((max(m, 1),), -1, dtype=torch.int32, device="cuda")  # noqa: E731
        torch.cuda.synchronize()
        try:
            if kind == "dist":
                same = p["sym"]  # one buffer on both sides, i < j
                cols = R if same else Q
                out = torch.empty(3 * (R * cols + 16), dtype=torch.int32, device="cuda")
                torch.cuda.synchronize()
                found, status = c.dist_block_dev(*rp, R, 0, *(rp if same else qp), cols, 0, D, K, same, self.th, out.data_ptr(), R * cols + 16)
                h = hits_of(hg, out, found)
                return status, found, np.sort(h, order=("ref_idx", "qry_idx")).tobytes()
            if kind == "dist_full":
                out = torch.empty(R * Q, dtype=torch.float32, device="cuda")
                c.dist_full_dev(*rp, R, *qp, Q, D, K, out.data_ptr())
                c.sync()
                return out.cpu().numpy().tobytes()
            if kind == "hamming":
                out = torch.empty(3 * R * Q, dtype=torch.int32, device="cuda")
                found, status = c.hamming_search_dev(self.rbits.data_ptr() + p["first"] * (D // 8), R, self.qbits.data_ptr(), Q, D, D // 2 - 8, out.data_ptr(), R * Q)
                h = out[:3 * found].cpu().numpy().view(hg.HAM_HIT_DTYPE)
                return status, found, np.sort(h, order=("ref_idx", "qry_idx")).tobytes()
            if kind == "pairs":
                ij = np.zeros(200, hg.ANI_HIT_DTYPE)
                ij["ref_idx"], ij["qry_idx"] = np.arange(200) % R, (np.arange(200) * 7) % Q
                d_ij, ani = up(ij), torch.zeros(800, dtype=torch.float32, device="cuda")
                torch.cuda.synchronize()
                c.ani_pairs_dev(*rp, R, *qp, Q, D, K, d_ij.data_ptr(), 200, ap.ALL, ani.data_ptr(), None)
                return ani.cpu().numpy().tobytes()
            rep, cl = i32(), i32()
            if kind == "uf":
                nc = c.cluster_dev(*cp_, n, D, rep.data_ptr(), cl.data_ptr(), K, 95.0)
                return nc, rep.cpu().numpy().tobytes(), cl.cpu().numpy().tobytes()
            if kind in ("greedy", "setcover"):
                fn = c.cluster_greedy_dev if kind == "greedy" else c.cluster_setcover_dev
                ani = torch.zeros(n, dtype=torch.float32, device="cuda")
                torch.cuda.synchronize()
                nc = fn(*cp_, n, D, rep.data_ptr(), cl.data_ptr(), ani.data_ptr(), K, 95.0)
                return nc, rep.cpu().numpy().tobytes(), cl.cpu().numpy().tobytes(), ani.cpu().numpy().tobytes()
            if kind == "tree":
                tree = torch.zeros(3 * n, dtype=torch.int32, device="cuda")
                torch.cuda.synchronize()
                ne, nc = c.cluster_tree_dev(*cp_, n, D, tree.data_ptr(), n - 1, rep.data_ptr(), cl.data_ptr(), K, 95.0)
                return ne, nc, tree[:3 * ne].cpu().numpy().tobytes(), rep.cpu().numpy().tobytes()
            if kind in ("average", "complete"):
                fn = c.cluster_average_dev if kind == "average" else c.cluster_complete_dev
                into, level, size = i32(), torch.zeros(n, dtype=torch.float32, device="cuda"), i32()
                torch.cuda.synchronize()
                nc = fn(*cp_, n, D, rep.data_ptr(), cl.data_ptr(), into.data_ptr(), level.data_ptr(), size.data_ptr(), K, 95.0)
                return (nc,) + tuple(t.cpu().numpy().tobytes() for t in (rep, cl, into, level, size))
            if kind in ("stats", "stats_bad"):
                ids = torch.arange(n, dtype=torch.int32, device="cuda") // 20
                k = (n + 19) // 20 - (kind == "stats_bad")
                node = torch.zeros(n * 24, dtype=torch.uint8, device="cuda")
                stat = torch.zeros(max(k, 1) * 48, dtype=torch.uint8, device="cuda")
                torch.cuda.synchronize()
                c.cluster_stats_dev(*cp_, n, D, ids.data_ptr(), k, node.data_ptr(), stat.data_ptr(), K)
                return node.cpu().numpy().tobytes(), stat.cpu().numpy().tobytes()
            if kind == "nj":
                out = torch.zeros((n - 1) * 24, dtype=torch.uint8, device="cuda")
                torch.cuda.synchronize()
                return c.nj_dev(*cp_, n, D, out.data_ptr(), K), out.cpu().numpy().tobytes()
            if kind == "search":
                out, cnt = torch.zeros(Q * 3 * 3, dtype=torch.int32, device="cuda"), torch.zeros(Q, dtype=torch.int32, device="cuda")
                torch.cuda.synchronize()
                c.search_topk_dev(*rp, R, *qp, Q, D, K, self.th, 3, out.data_ptr(), cnt.data_ptr())
                c.sync()
                return out.cpu().numpy().tobytes(), cnt.cpu().numpy().tobytes()
            if kind == "abandon_bad":
                bad = np.zeros(4, hg.ANI_HIT_DTYPE)
                bad["qry_idx"], bad["ani"] = (1, 2, n, 3), 99.0
                d_bad = up(bad)
                torch.cuda.synchronize()
                c.cluster_init_dev(rep.data_ptr(), n)
                c.cluster_add_hits_dev(rep.data_ptr(), n, d_bad.data_ptr(), 4, 95.0)
                c.sync()
                return None
        except hg.HgError as e:
            return "status %d" % e.status
        raise AssertionError(kind)


def test_f_seeded_soak_against_fresh_contexts(hg, orc, session):
    soak = Soak(hg, orc)
    rng = np.random.default_rng(SOAK_SEED)
    calls = [soak.params(rng) for _ in range(SOAK_CALLS)]
    t0 = time.time()
    for n, p in enumerate(calls):
        got = soak.run(session.ctx, p)
        with hg.Context(0) as fresh:
            want = soak.run(fresh, p)
        if got != want:
            print("section f: seed %d, call %d differs; the calls up to it:" % (SOAK_SEED, n))
            for q in calls[:n + 1]:
                print("   ", q)
        assert got == want, (SOAK_SEED, n, p)
    timed("f", t0, calls=len(calls), kinds=len({p["kind"] for p in calls}))
