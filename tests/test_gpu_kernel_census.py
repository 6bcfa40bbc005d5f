"""Every compiled dist and k-mer kernel (tests/kernel_census.py), run by the input its census row names, checked two ways: the
call reports that kernel (ctx.last_kernel), and its result equals a plain exact reference bit for bit -- int64 dot products
(containment_ref.exact_dots) with the oracle's float32 ANI (containment_ref.ani_ref), the oracle's Hamming distances, the
oracle's sampled hash sets.

Inputs of every MFMA dist row: ragged shapes (R = 300, Q = 270 as two sets, 333 rows compared with themselves in one buffer),
sketch-like HVs of graded completeness (containment_ref.fragment_hvs) with an all-zero row and a row duplicated in the other
set, thresholds on a value of the reference matrix, one float32 ulp either side of it, 0 and -3 (every pair), 100 and 100.5,
k = 1, 21, 255; symmetric calls for the Mash-style and max containment metrics (containment must refuse them).  The windowed
rows run three window classes, each asserted on the host with the prepass's bound (a product of maxima <= 2^48, per window of
64 << c dims): the 2 048-dim window (verdict 1), the 1 024-dim window (verdict 2) and the non-speculative rerun (windows of
512 dims, and of 64 dims with rows whose norm exceeds 2^29).
"""
import numpy as np
import pytest
import torch

import containment_ref as cr
import kernel_census as kc

pytestmark = pytest.mark.gpu
KS = (1, 21, 255)
D = 4096
MAX = 2**64 - 1
METRICS = {"mash": (cr.MASH,), "ctm": (cr.CONTAINMENT, cr.MAX_CONTAINMENT), "any": (cr.MASH, cr.CONTAINMENT, cr.MAX_CONTAINMENT)}
WIN_CLASSES = ("v1", "v2", "r512", "r64")  # verdict 1, verdict 2, rerun on 512-dim windows, rerun on 64-dim windows
ACGT = np.frombuffer(b"ACGT", np.uint8)
COMP = np.zeros(256, np.uint8)
COMP[list(b"ACGT")] = list(b"TGCA")


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
    """the module's ctx, back on the default paths and metric after each test"""
    yield mctx
    for key in ("dist_path", "dist_tile", "ham_path", "hostfed"):
        mctx.set_debug(key, "")
    mctx.set_ani_metric(cr.MASH)


# ---- the window a raw-value operand set needs (raw_prepass / prep_fast_kernel / decide_kernel, on the host) ----------
def window_class(r, q):
    """(verdict, c): verdict 0 = one window covers K, 1 / 2 = windows of 2 048 / 1 024 dims, 3 = the rerun, whose c is the
    largest window 64 << c that is safe; 'int' when some |x| > 2048"""
    def stats(h):
        x = np.asarray(h, np.int64)
        sq = x * x
        return int(np.abs(x).max()), [int(sq.reshape(len(x), -1, 64 << c).sum(2).max()) for c in range(7)]
    mr, wr = stats(r)
    mq, wq = stats(q)
    if mr > 2048 or mq > 2048:
        return "int", None
    safe = [wr[c] * wq[c] <= 1 << 48 for c in range(7)]
    verdict = 0 if safe[6] else 1 if safe[5] else 2 if safe[4] else 3
    return verdict, max([c for c in range(7) if safe[c]], default=-1)


# ---- input sets ---------------------------------------------------------------------------------------------------------
class Pair:
    def __init__(self, r, q=None):
        self.same = q is None
        self.r = np.ascontiguousarray(r, np.int16)
        self.q = self.r if self.same else np.ascontiguousarray(q, np.int16)
        self.rn = cr.norms(self.r)
        self.qn = self.rn if self.same else cr.norms(self.q)
        self.dots = cr.exact_dots(self.r, self.q)
        self.cls = window_class(self.r, self.q)


def with_edges(hv):
    """R / Q of a family set: an all-zero row in each, one row of R duplicated in Q; and the 333-row self set"""
    r, q, s = hv[:300].copy(), hv[300:570].copy(), hv[:333].copy()
    r[5] = 0
    q[0] = 0
    q[7] = r[3]
    s[4] = 0
    s[20] = s[2]
    return [Pair(r, q), Pair(s)]


_SETS = {}


def sets(kind):
    if kind not in _SETS:
        if kind == "sketch":
            hv, _, _ = cr.fragment_hvs(570, D, seed=11)
            _SETS[kind] = with_edges(hv)
        elif kind == "stress":
            r, _, q, _ = cr.stress_hvs(260, 290, D, seed=3, blocks=20, block_hashes=100)
            _SETS[kind] = [Pair(r, q)]
        elif kind == "wide":  # values beyond f16's exact integers: the integer kernel
            hv, _, _ = cr.fragment_hvs(570, D, seed=12)
            hv[2, 10], hv[2, 11], hv[310, 0] = 3000, -2049, 2500
            _SETS[kind] = with_edges(hv)
        elif kind in WIN_CLASSES:
            bh = {"v1": 150, "v2": 300, "r512": 560, "r64": 560}[kind]
            hv, _, _ = cr.fragment_hvs(570, D, seed=13 + WIN_CLASSES.index(kind), block_hashes=bh)
            if kind == "r64":  # rows of norm 400^2 * 4096 > 2^29: the pre-filter's "phase 1 decides" words
                rng = np.random.default_rng(77)
                hv[[10, 11, 320]] = rng.choice(np.array([-400, 400], np.int16), (3, D))
            _SETS[kind] = with_edges(hv)
        else:
            raise KeyError(kind)
    return _SETS[kind]


WANT_CLASS = {"sketch": (0, 6), "stress": (0, 6), "v1": (1, 5), "v2": (2, 4), "r512": (3, 3), "r64": (3, 0), "wide": ("int", None)}


def thresholds(ani):
    vals = np.sort(ani[(ani > 0) & (ani < 100)].ravel())
    v = vals[vals.size // 2] if vals.size else np.float32(50)
    up, down = np.nextafter(v, np.float32(np.inf)), np.nextafter(v, np.float32(-np.inf))
    return [float(np.float32(t)) for t in (v, up, down, 0.0, -3.0, 100.0, 100.5)]


def assert_same_hits(got, ani, th, symmetric, what):
    m = ani >= np.float32(th)
    if symmetric:
        m &= np.triu(np.ones(m.shape, bool), 1)
    i, j = np.nonzero(m)
    Q = ani.shape[1]
    key = got["ref_idx"].astype(np.int64) * Q + got["qry_idx"].astype(np.int64)
    assert np.unique(key).size == key.size, ("duplicate hits", what)
    order = np.argsort(key)
    assert key.size == i.size and (key[order] == i.astype(np.int64) * Q + j).all(), (what, key.size, i.size)
    assert (got["ani"][order].view(np.uint32) == ani[i, j].view(np.uint32)).all(), what


def run_dist(hg, ctx, orc, row, p, metric):
    """every k and threshold (and symmetric form) of one input pair under one metric"""
    ctx.set_ani_metric(metric)
    for k in KS:
        ani = cr.ani_ref(orc, p.dots, p.rn[:, None], p.qn[None, :], k, metric)
        if row.entry == "dist_full":
            got = ctx.dist_full(p.r, p.rn, p.q, p.qn, k)
            assert ctx.last_kernel("dist") == row.name, (ctx.last_kernel("dist"), metric, k)
            assert (got.view(np.uint32) == ani.view(np.uint32)).all(), (row.name, metric, k)
            continue
        for sym in ((False, True) if p.same else (False,)):
            if sym and metric == cr.CONTAINMENT:
                with pytest.raises(hg.HgError) as e:
                    ctx.dist(p.r, p.rn, p.q, p.qn, k, symmetric=True, ani_th=90.0)
                assert e.value.status == hg.ERR_INVALID
                continue
            for th in thresholds(ani):
                what = (row.name, metric, k, sym, th, p.r.shape[0], p.q.shape[0])
                got = ctx.dist(p.r, p.rn, p.q, p.qn, k, symmetric=sym, ani_th=th, cap=p.r.shape[0] * p.q.shape[0] + 16)
                assert ctx.last_kernel("dist") == row.name, (ctx.last_kernel("dist"),) + what
                assert_same_hits(got, ani, th, sym, what)


# ---- 1. every dist instantiation ------------------------------------------------------------------------------------
DIST_MFMA = [r for r in kc.DIST_ROWS if r.entry in ("dist", "dist_full") and r.name.startswith("dist_mfma")]


@pytest.mark.parametrize("row", DIST_MFMA, ids=[r.name for r in DIST_MFMA])
def test_dist_mfma_row(hg, ctx, orc, row):
    for key, val in row.debug.items():
        ctx.set_debug(key, val)
    kinds = list(WIN_CLASSES) if row.inputs == "win" else ["sketch"]
    if row.metric == "ctm" and row.inputs == "sketch" and row.debug.get("dist_tile") in ("big", "wide"):
        kinds.append("stress")  # big tiles: containment hits the Mash-style bound would cut
    for kind in kinds:
        for p in sets(kind):
            assert p.cls == WANT_CLASS[kind], (kind, p.cls)
            for metric in METRICS[row.metric]:
                run_dist(hg, ctx, orc, row, p, metric)


def test_skinny_rows(hg, ctx, orc):
    """dist_skinny_kernel<false> (<= 16 query rows) and <true> (<= 16 reference rows), no hooks"""
    rows = {r.inputs: r for r in kc.DIST_ROWS if r.name.startswith("dist_skinny")}
    pr, = [p for p in sets("sketch") if not p.same]
    cases = [("skinny_q", Pair(pr.r, pr.q[:16])), ("skinny_q", Pair(pr.q[:12])), ("skinny_r", Pair(pr.r[:5], pr.q))]
    for inputs, p in cases:
        for metric in METRICS["any"]:
            run_dist(hg, ctx, orc, rows[inputs], p, metric)


def test_int_row(hg, ctx, orc):
    """dist_int_kernel: some |x| > 2048, thresholded and full"""
    row, = [r for r in kc.DIST_ROWS if r.name == "dist_int_kernel"]
    full = row._replace(entry="dist_full")
    for p in sets("wide"):
        assert p.cls[0] == "int"
        for metric in METRICS["any"]:
            run_dist(hg, ctx, orc, row, p, metric)
            run_dist(hg, ctx, orc, full, p, metric)


HAM = [r for r in kc.DIST_ROWS if r.entry == "hamming"]


@pytest.mark.parametrize("row", HAM, ids=[r.name for r in HAM])
def test_hamming_row(ctx, orc, row):
    for key, val in row.debug.items():
        ctx.set_debug(key, val)
    dims = (4096, 1000) if row.debug["ham_path"] == "fp4" else (4096, 384)  # (byte operands: hv_d % 128 == 0)
    for d in dims:
        hv, _, _ = cr.fragment_hvs(570, d, seed=21, blocks=10, block_hashes=40)
        hv[5] = 0
        hv[300 + 7] = hv[3]
        for rb, qb in ((orc.binarize(hv[:300]), orc.binarize(hv[300:570])), (orc.binarize(hv[:333]), None)):
            same = qb is None
            qb = rb if same else qb
            want = orc.hamming_matrix(rb, qb).astype(np.int64)
            dr = torch.from_numpy(rb.view(np.int32)).cuda()
            dq = dr if same else torch.from_numpy(qb.view(np.int32)).cuda()
            R, Q = rb.shape[0], qb.shape[0]
            hits = torch.empty(3 * (R * Q + 16), dtype=torch.int32, device="cuda:0")
            w = rb.shape[1] * 32
            med = int(np.median(want))
            for md in (med, med - 1, med + 1, 0, w - 1, w, w + 7):
                n, st = ctx.hamming_search_dev(dr.data_ptr(), R, dq.data_ptr(), Q, d, md, hits.data_ptr(), R * Q + 16)
                assert st == 0 and ctx.last_kernel("dist") == row.name, (ctx.last_kernel("dist"), d, md)
                got = hits[: 3 * n].cpu().numpy().view(np.uint32).reshape(-1, 3).astype(np.int64)
                i, j = np.nonzero(want <= md)
                key = np.sort(got[:, 0] * Q + got[:, 1])
                assert n == i.size and (key == i * Q + j).all(), (row.name, d, md, same, n, i.size)
                assert (got[:, 2] == want[got[:, 0], got[:, 1]]).all(), (row.name, d, md, same)


def test_windowed_launch_reports_its_name(ctx, orc):
    """a thresholded call on sketches that need 2 048- or 1 024-dim windows, no hooks: the guarded windowed kernel does the
    work and last_kernel("dist") names it, not the whole-K kernel queued in front of it"""
    want = kc.mfma_name(True, False, False, False, 4)
    for kind in ("v1", "v2"):
        p, = [p for p in sets(kind) if not p.same]
        assert p.cls == WANT_CLASS[kind]
        ani = cr.ani_ref(orc, p.dots, p.rn[:, None], p.qn[None, :], 21, cr.MASH)
        th = thresholds(ani)[0]
        got = ctx.dist(p.r, p.rn, p.q, p.qn, 21, ani_th=th, cap=p.r.shape[0] * p.q.shape[0])
        assert ctx.last_kernel("dist") == want, (kind, ctx.last_kernel("dist"))
        assert_same_hits(got, ani, th, False, kind)


# ---- 2. every k-mer instantiation -----------------------------------------------------------------------------------
_SEQS = {}


def kmer_seq(k):
    """~20 kbp, seeded: lowercase, N runs, IUPAC bytes and, for odd k <= 32, planted k-mers whose two strands share their
    first (k - 1) / 2 bases (half + middle base + reverse complement of half)"""
    if k not in _SEQS:
        rng = np.random.default_rng(9900 + k)
        L = 20_000
        s = rng.choice(ACGT, L)
        if k % 2 == 1 and k <= 32:
            h = (k - 1) // 2
            for at in rng.integers(0, L - k, 150):
                half = rng.choice(ACGT, h)
                s[at:at + k] = np.concatenate([half, rng.choice(ACGT, 1), COMP[half[::-1]]])
        low = rng.random(L) < 0.04
        low[6000:6400] = True
        s[low] = s[low] + 32  # (all ACGT so far: a, c, g, t)
        for at in rng.integers(0, L - 60, 6):
            s[at:at + int(rng.integers(1, 50))] = ord("N")
        iu = np.frombuffer(b"RYKMSWBDHVn", np.uint8)
        pos = rng.integers(0, L, 60 if k <= 32 else 8)
        s[pos] = rng.choice(iu, pos.size)
        _SEQS[k] = s
    return _SEQS[k]


def run_kmer(ctx, orc, row, k, canonical):
    s = kmer_seq(k)
    u = orc.kmer_hash_sample(s, k, seed=123, canonical=canonical, threshold=MAX)
    assert u.size >= 1, (k, canonical)
    t = int(u[max(1, u.size // 3)]) if u.size > 1 else int(u[0])  # one of the sequence's own hashes: `<` keeps it out
    want = orc.kmer_hash_sample(s, k, seed=123, canonical=canonical, threshold=t)
    assert want.size == max(1, u.size // 3) if u.size > 1 else want.size == 0
    got = ctx.kmer_hash_sample(s, k, seed=123, canonical=canonical, threshold=t, cap=u.size + 64)
    assert ctx.last_kernel("kmer") == row.name, (ctx.last_kernel("kmer"), k, canonical)
    got = np.sort(got)
    assert got.size == want.size and (got == want).all(), (row.name, k, canonical, got.size, want.size)


@pytest.mark.parametrize("row", kc.KMER_ROWS, ids=[r.name for r in kc.KMER_ROWS])
def test_kmer_row(ctx, orc, row):
    ctx.set_debug("hostfed", row.debug["hostfed"])
    if row.name.startswith("kmer_sample_shared"):
        k, canonical = row.inputs
        run_kmer(ctx, orc, row, k, canonical)
    else:
        for k in row.inputs:
            for canonical in (False, True):
                run_kmer(ctx, orc, row, k, canonical)
