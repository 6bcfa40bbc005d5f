"""The dist path's exactness decisions, each at its constant (tests/dist_boundary_craft.py builds the inputs,
tests/dist_prep_model.py says what the prepasses must decide, tests/test_dist_prep_model.py proves on the host that every
input sits where this file needs it).

Every result is compared bit for bit with int64 dot products (containment_ref.exact_dots) and the oracle's float32 ANI
(containment_ref.ani_ref): the hit set equals the reference matrix cut at the threshold -- a value of that matrix, one
float32 ulp either side of it, and 0 -- without duplicates and with equal ANI bits; hg_ctx_last_dist_path and
hg_ctx_last_kernel("dist") are the model's.

  a. byte operands: c = +-127, +-128, +-254 (exact, path 1) and +-255 (vetoed) at the first / last dimension and both sides of
     a load and a chunk, at hv_d 512, 4056, 4096, 8192, on either side and both; the 16-bit wrap; a row whose x[0] alone is odd
  b. 0, 1, 2, 15, 16 entries per row (path 1: the first-entry fast path alone, and the further-entries loop), 17, 255, 256,
     257, every dimension (vetoed); two sets, one buffer, symmetric
  c. row and column clamped at the same dimensions, equal and opposite signs, the diagonal of a self-comparison
  d. hits that the corrections alone decide, with the phase-0 slack attained: every metric, parity combination, k and tile
  e. hg_dist_prep_ops_dev's bytes, records and flag against the model; the inputs of a-d through hg_dist_block_ops_dev with one
     to three owners: a at all four hv_d, d under every metric, parity combination, k and tile
  f. centred f16: c = +-2048 / +-2049, sum c^2 products of exactly 2^48 with dot products of +-2^24 in c, mixed parity
  g. raw f16: |x| = 2048 / 2049, the whole-row, 2 048- and 1 024-window products at 2^48 and one above, the extremal row in
     every statistics slot position, hv_d without window statistics, the fast prepass's lane sums at their largest
"""
import functools
import zlib

import numpy as np
import pytest
import torch

import containment_ref as cr
import dist_boundary_craft as C
import dist_prep_model as M
import kernel_census as kc

pytestmark = pytest.mark.gpu
METRICS = (cr.MASH, cr.CONTAINMENT, cr.MAX_CONTAINMENT)


@pytest.fixture(scope="module")
def hg():
    import hypergen_amd
    return hypergen_amd


@pytest.fixture(scope="module")
def mctx(hg):
    c = hg.Context(0)
    yield c
    c.close()


@pytest.fixture
def ctx(mctx):
    yield mctx
    for key in ("dist_path", "dist_tile"):
        mctx.set_debug(key, "")
    mctx.set_ani_metric(cr.MASH)


class Dots:
    """exact_dots of sets that differ from a base pair in a few rows: only those rows and columns are formed again"""

    def __init__(self, r, q):
        self.r, self.q, self.d = r.copy(), q.copy(), cr.exact_dots(r, q)

    def of(self, r, q):
        if r.shape != self.r.shape or q.shape != self.q.shape:
            return cr.exact_dots(r, q)
        ri, qi = np.nonzero((r != self.r).any(1))[0], np.nonzero((q != self.q).any(1))[0]
        if ri.size + qi.size > 40:
            return cr.exact_dots(r, q)
        d = self.d.copy()
        if qi.size:
            d[:, qi] = cr.exact_dots(r, q[qi])
        if ri.size:
            d[ri, :] = cr.exact_dots(r[ri], q)
        return d


_EXACT = {}


def exact_of(case, r, q):
    """the input's int64 dot products, formed once for the tests that run the same input (sections a-c and e)"""
    key = (case.name, r.shape, q.shape, zlib.crc32(r.tobytes()), zlib.crc32(q.tobytes()))
    if key not in _EXACT:
        _EXACT[key] = cr.exact_dots(r, q)
    return _EXACT[key]


def thresholds(ani):
    vals = np.sort(ani[(ani > 0) & (ani < 100)].ravel())
    v = vals[vals.size // 2] if vals.size else np.float32(50)
    return [float(np.float32(t)) for t in (v, np.nextafter(v, np.float32(np.inf)), np.nextafter(v, np.float32(-np.inf)), 0.0)]


def assert_same_hits(got, ani, th, symmetric, what):
    m = ani >= np.float32(th)
    if symmetric:
        m &= np.triu(np.ones(m.shape, bool), 1)
    i, j = np.nonzero(m)
    Q = ani.shape[1]
    key = got["ref_idx"].astype(np.int64) * Q + got["qry_idx"].astype(np.int64)
    assert np.unique(key).size == key.size, ("duplicate hits", what)
    order = np.argsort(key)
    want = i.astype(np.int64) * Q + j
    assert key.size == i.size and (key[order] == want).all(), ("hit set", what, key.size, i.size, np.setxor1d(key, want)[:8].tolist())
    assert (got["ani"][order].view(np.uint32) == ani[i, j].view(np.uint32)).all(), ("ANI bits", what)


def run_case(ctx, orc, case, dist_path, tile, dots=None, metric=cr.MASH, k=21, ths=None, entries=("dist",), clean=None):
    """one crafted input under one route: path, kernel and hits at every threshold; returns the path.  clean: an input of the same
    shape that the byte path accepts, run in front of every thresholded call: the call on the same buffers right after a
    successful byte-path call trusts that path and queues no fallback, so a veto there is rerun through the f16 schedule"""
    same = case.q is None
    r = np.ascontiguousarray(case.r)
    q = r if same else np.ascontiguousarray(case.q)
    rn = cr.norms(r)
    qn = rn if same else cr.norms(q)
    d = dots.of(r, q) if dots is not None else exact_of(case, r, q)
    ani = cr.ani_ref(orc, d, rn[:, None], qn[None, :], k, metric)
    ctx.set_debug("dist_path", dist_path)
    ctx.set_debug("dist_tile", tile)
    ctx.set_ani_metric(metric)
    path = None
    for entry in entries:
        want_path, want_kernel = M.expect_dist(r, q, dist_path, tile, metric, entry)
        what = (case.name, dist_path, tile, metric, k, entry)
        if entry == "dist_full":
            got = ctx.dist_full(r, rn, q, qn, k)
            assert ctx.last_kernel("dist") == want_kernel, (ctx.last_kernel("dist"), want_kernel) + what
            assert (got.view(np.uint32) == ani.view(np.uint32)).all(), what
            continue
        for th in (thresholds(ani) if ths is None else ths):
            if clean is not None:
                ctx.dist(clean.r, cr.norms(clean.r), clean.q, cr.norms(clean.q), k, symmetric=False, ani_th=th, cap=r.shape[0] * q.shape[0] + 16)
                assert ctx.last_dist_path() == 1, ("clean call in front of",) + what
            got = ctx.dist(r, rn, q, qn, k, symmetric=case.sym, ani_th=th, cap=r.shape[0] * q.shape[0] + 16)
            assert (ctx.last_dist_path(), ctx.last_kernel("dist")) == (want_path, want_kernel), (ctx.last_dist_path(), ctx.last_kernel("dist"), want_path, want_kernel, th) + what
            assert_same_hits(got, ani, th, case.sym, what + (th,))
        path = want_path
    return path


# ---- a ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def clamp_dots(hv_d, e):
    """the exact dot products of the clamp inputs' base sets, formed once for sections a and e"""
    return Dots(*C.two_sets(hv_d, e, e, 100 + hv_d + e))


@pytest.mark.parametrize("e", (0, 1))
@pytest.mark.parametrize("hv_d", C.HV_DS)
def test_i8_clamp_and_residual(ctx, orc, hv_d, e):
    dots = clamp_dots(hv_d, e)
    tile = "wide" if (hv_d // 8 + e) % 2 else "big"
    ok = None
    for case in C.clamp_cases(hv_d, e):  # ok, veto, veto per side: the side's exact input runs in front of every vetoed call
        veto = "veto" in case.name
        ok = ok if veto else case
        path = run_case(ctx, orc, case, "i8", tile, dots, clean=ok if veto else None)
        assert path == (0 if veto else 1), case.name


def test_i8_wrap_and_parity(ctx, orc):
    clean = C.Case("clean", *C.two_sets(4096, 1, 1, 139), False)
    assert run_case(ctx, orc, clean, "i8", "big") == 1
    for case, want in zip(C.wrap_cases(), (2, 2, 0)):
        assert run_case(ctx, orc, case, "i8", "big", clean=clean) == want, case.name


# ---- b, c ---------------------------------------------------------------------------------------------------------------
def test_i8_entries_per_row(ctx, orc):
    for n, case in enumerate(C.entries_cases()):
        path = run_case(ctx, orc, case, "i8", "wide" if n % 2 else "big")
        assert path == (0 if "veto" in case.name else 1), case.name


def test_i8_coinciding_entries(ctx, orc):
    for n, case in enumerate(C.coincide_cases()):
        assert run_case(ctx, orc, case, "i8", "wide" if n % 2 else "big") == 1, case.name


# ---- d ------------------------------------------------------------------------------------------------------------------
def decided_thresholds(ani, n):
    """the exact ANI of three rescued and three demoted pairs (rotating with n) and the next float above each"""
    out = []
    for t in range(3):
        i = C.RP[(n + 3 * t) % 8]
        for j in (C.QP[(n + 5 * t + 1) % 8], C.QM[(n + 7 * t + 2) % 8]):
            v = ani[i, j]
            out += [float(v), float(np.nextafter(v, np.float32(np.inf)))]
    return out


@pytest.mark.parametrize("er,eq", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_i8_hits_decided_by_the_corrections(ctx, orc, er, eq):
    r, q = C.decided_sets(er, eq)
    case = C.Case("decided-%d%d" % (er, eq), r, q, False)
    dots = Dots(r, q)
    n = 0
    for metric in METRICS:
        for k in (21, 255):
            d = dots.of(r, q)
            ani = cr.ani_ref(orc, d, cr.norms(r)[:, None], cr.norms(q)[None, :], k, metric)
            for tile in ("big", "wide"):
                assert run_case(ctx, orc, case, "i8", tile, dots, metric, k, decided_thresholds(ani, n)) == 1
                n += 1


# ---- e ------------------------------------------------------------------------------------------------------------------
def prep_ops(hg, c, hv):
    """hg_dist_prep_ops_dev on the rows of hv: (ops, meta, flag) tensors"""
    rows, hv_d = hv.shape
    rb, mb = hg.lib().hg_dist_ops_row_bytes(hv_d), hg.lib().hg_dist_ops_meta_bytes()
    t = torch.from_numpy(np.ascontiguousarray(hv)).cuda()
    ops = torch.full((rows, rb), 0x5A, dtype=torch.uint8, device="cuda")
    meta = torch.full((rows, mb), 0x5A, dtype=torch.uint8, device="cuda")
    flag = torch.full((1,), 77, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()  # (the fills run on torch's stream, the library on the context's own: without this a fill may land last)
    c.dist_prep_ops_dev(t.data_ptr(), rows, hv_d, ops.data_ptr(), meta.data_ptr(), flag.data_ptr())
    c.sync()
    return ops, meta, flag


def assert_prep_equals_model(hg, c, hv, what):
    ops, meta, flag = prep_ops(hg, c, hv)
    m = M.i8_rows(hv)
    hv_d = hv.shape[1]
    kp8 = (hv_d + 127) // 128 * 128
    a = np.zeros((hv.shape[0], kp8), np.int8)
    a[:, :hv_d] = m.a
    assert (ops.cpu().numpy().view(np.int8)[:, :kp8] == a).all(), ("byte operands", what)
    rec = meta.cpu().numpy().view(np.int32).reshape(hv.shape[0], 2 + M.I8_ROW_SLOTS)
    assert (rec[:, 0] == m.info).all(), ("info", what)
    assert int(flag[0]) == M.i8_flag(m), ("flag", what, int(flag[0]), M.i8_flag(m))
    for i in range(hv.shape[0]):
        if m.slot[i] is not None:
            assert int(rec[i, 1]) == m.slot[i], ("slot", what, i, int(rec[i, 1]), m.slot[i])
        n_st = min(int(m.n[i]), M.I8_ROW_SLOTS)
        words = {M.ent_word(d, b) for d, b in m.ents[i]}
        got = [int(w) & 0xFFFFFFFF for w in rec[i, 2:2 + n_st]]
        assert len(set(got)) == n_st and set(got) <= words and (int(m.n[i]) > M.I8_ROW_SLOTS or set(got) == words), ("entries", what, i)
        assert (rec[i, 2 + n_st:] == 0).all(), ("unused entry slots", what, i)


def block_ops_case(hg, c, orc, case, world, ths=None, k=21, metric=cr.MASH, tile="big", dots=None):
    """the case's reference rows prepared by `world` owners, gathered, compared by hg_dist_block_ops_dev under the ctx's metric:
    ERR_INEXACT exactly where the model vetoes, else the hits of the exact reference; returns the model's verdict"""
    from hypergen_amd import shard
    r = np.ascontiguousarray(case.r)
    q = r if case.q is None else np.ascontiguousarray(case.q)
    Rn, Qn, hv_d = r.shape[0], q.shape[0], r.shape[1]
    rn, qn = cr.norms(r), cr.norms(q)
    ani = cr.ani_ref(orc, dots.of(r, q) if dots is not None else exact_of(case, r, q), rn[:, None], qn[None, :], k, metric)
    ok = M.i8_ok(hv_d, M.i8_rows(r), M.i8_rows(q))
    ctm = metric != cr.MASH
    want_kernel = kc.mfma_name(False, False, True, True, 4 if ctm or tile != "wide" else 5, i8=True, ctm=ctm)
    c.set_debug("dist_tile", tile)
    c.set_ani_metric(metric)
    ranges = [shard.shard_range(Rn, w, world) for w in range(world)]
    parts = [prep_ops(hg, c, r[lo:hi]) for lo, hi in ranges]
    flags = torch.cat([p[2] for p in parts]).contiguous()
    for (lo, hi), p in zip(ranges, parts):
        assert int(p[2][0]) == M.i8_flag(M.i8_rows(r[lo:hi])), (case.name, lo, hi)
    Rp = hg.lib().hg_dist_ops_padded_rows(Rn)
    ops = torch.full((Rp, parts[0][0].shape[1]), 0x5A, dtype=torch.uint8, device="cuda")
    ops[:Rn] = torch.cat([p[0] for p in parts])
    meta = torch.cat([p[1] for p in parts]).contiguous()
    t_rn, t_q, t_qn = torch.from_numpy(rn).cuda(), torch.from_numpy(q).cuda(), torch.from_numpy(qn).cuda()
    cap = Rn * Qn + 16
    hits = torch.empty(cap * 3, dtype=torch.int32, device="cuda")
    for th in (thresholds(ani) if ths is None else ths):
        what = (case.name, "block_ops", world, metric, k, tile, th)
        found, st = c.dist_block_ops_dev(ops.data_ptr(), meta.data_ptr(), t_rn.data_ptr(), Rn, 0, 0, flags.data_ptr(), world,
                                         t_q.data_ptr(), t_qn.data_ptr(), Qn, 0, hv_d, k, case.sym, th, hits.data_ptr(), cap)
        if not ok:
            assert st == hg.ERR_INEXACT and found == 0, what + (st,)
            continue
        assert st == 0 and (c.last_dist_path(), c.last_kernel("dist")) == (1, want_kernel), what + (st, c.last_dist_path(), c.last_kernel("dist"))
        got = np.zeros(found, hg.ANI_HIT_DTYPE)
        raw = hits[: 3 * found].cpu().numpy().reshape(-1, 3)
        got["ref_idx"], got["qry_idx"], got["ani"] = raw[:, 0], raw[:, 1], raw[:, 2].view(np.float32)
        assert_same_hits(got, ani, th, case.sym, what)
    return ok


def test_prepared_operands_equal_the_model(hg, ctx):
    for hv_d in C.HV_DS:
        for e in (0, 1):
            for case in C.clamp_cases(hv_d, e):
                assert_prep_equals_model(hg, ctx, case.r, (case.name, hv_d, e, "r"))
                assert_prep_equals_model(hg, ctx, case.q, (case.name, hv_d, e, "q"))
    for case in C.wrap_cases() + C.entries_cases() + C.coincide_cases():
        for hv, side in ((case.r, "r"), (case.q, "q")):
            if hv is not None:
                assert_prep_equals_model(hg, ctx, hv, (case.name, side))
    # every boundary value at every boundary dimension in a row of its own, one launch per row: the flag is the row's alone
    for hv_d in C.HV_DS:
        for e in (0, 1):
            base = C.two_sets(hv_d, e, e, 700 + e, r=1, q=1)[0]
            for c in C.CLAMP_OK + (255, -255, 256, -256):
                for d in C.bdims(hv_d):
                    hv = base.copy()
                    C.set_c(hv, 0, d, c)
                    assert_prep_equals_model(hg, ctx, hv, ("single", hv_d, e, c, d))
    for hv, name in ((np.array([[32767, 1, 3, 5, 7, 9, 11, 13]], np.int16), "wrap"), (np.array([[-32768, 0, 2, 4, 6, 8, 10, 12]], np.int16), "min")):
        assert_prep_equals_model(hg, ctx, hv, name)


@pytest.mark.parametrize("e", (0, 1))
@pytest.mark.parametrize("hv_d", C.HV_DS)
def test_clamp_cases_through_block_ops(hg, ctx, orc, hv_d, e):
    """section a through the prepared-operand route, at every hv_d: with and without bytes in the 128-byte K padding, and at the
    byte path's upper limit"""
    vetoed = 0
    for n, case in enumerate(C.clamp_cases(hv_d, e)):
        vetoed += not block_ops_case(hg, ctx, orc, case, 1 + (n + e) % 3, tile=("big", "wide")[(n + hv_d // 8) % 2], dots=clamp_dots(hv_d, e))
    assert vetoed == 6


def test_prepared_operands_through_block_ops(hg, ctx, orc):
    """sections a (16-bit wrap, lone odd x[0]), b and c through the prepared-operand route"""
    vetoed = 0
    cases = C.wrap_cases() + C.entries_cases() + C.coincide_cases()
    for n, case in enumerate(cases):
        vetoed += not block_ops_case(hg, ctx, orc, case, 1 + n % 3, tile=("big", "wide")[n % 2])
    assert vetoed == 3 + sum("veto" in c.name for c in cases)


@pytest.mark.parametrize("er,eq", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_decided_hits_through_block_ops(hg, ctx, orc, er, eq):
    """section d through the prepared-operand route: every metric, k and tile, thresholds at the decided pairs' exact ANI"""
    r, q = C.decided_sets(er, eq)
    case = C.Case("decided-%d%d" % (er, eq), r, q, False)
    dots = Dots(r, q)
    n = 0
    for metric in METRICS:
        for k in (21, 255):
            ani = cr.ani_ref(orc, dots.of(r, q), cr.norms(r)[:, None], cr.norms(q)[None, :], k, metric)
            for tile in ("big", "wide"):
                assert block_ops_case(hg, ctx, orc, case, 1 + n % 3, decided_thresholds(ani, n), k, metric, tile, dots)
                n += 1


# ---- f, g ---------------------------------------------------------------------------------------------------------------
def test_centred_f16_boundaries(ctx, orc):
    for n, case in enumerate(C.cen_cases()):
        path = run_case(ctx, orc, case, "cen", "wide" if n % 2 else "big")
        fallback = any(s in case.name for s in ("2049", "65", "mixed"))
        assert (path != 3) == fallback, (case.name, path)


def test_raw_f16_chain_boundaries(ctx, orc):
    for n, case in enumerate(C.raw_cases()):
        path = run_case(ctx, orc, case, "f16", "wide" if n % 2 else "big", entries=("dist", "dist_full"))
        assert path == (2 if case.name == "raw-2049" else 0), case.name


def test_raw_f16_extremal_row_in_every_slot(ctx, orc):
    r, q = C.slot_sets()
    dots = Dots(r, q)
    for above in (False, True):
        for row in C.SLOT_ROWS:
            r2 = r.copy()
            r2[row] = C.slot_row(above)
            case = C.Case("slot-%d-%s" % (row, "above" if above else "at"), r2, q, False)
            d = dots.of(r2, q)
            ani = cr.ani_ref(orc, d, cr.norms(r2)[:, None], cr.norms(q)[None, :], 21, cr.MASH)
            th = float(np.sort(ani[row])[35])  # a value of the extremal row
            assert run_case(ctx, orc, case, "f16", "big", dots, ths=[th, 0.0]) == 0
