"""The exactness decisions of the dist path restated on the host: what the operand prepasses of hg_dist_prep.h compute per row
and decide per call, the terms of the byte-operand identity per pair with the epilogue's phase-0 slack, and which path and
kernel a call then takes (the host logic of hg_run_dist, for problems small enough that the debug key picks the attempt).

Plain numpy in int64; nothing here calls the library.  tests/test_dist_prep_model.py checks it against Python loops,
tests/test_gpu_dist_boundaries.py checks the device against it.

Centred byte operands (prep_i8_kernel): a row's parity is e = x[0] & 1 and x = 2 c - e, so c = (x + e) >> 1; the operand is
a = clip(c, -127, 127), the residual b = c - a one "entry" (d, b) per clamped dimension, S = sum c, and
    dot(r, q) = 4 G - 2 e_q S_r - 2 e_r S_q + D e_r e_q + 4 sum_d b_r c_q + 4 sum_d a_r b_q,      G = sum a_r a_q.
The kernel forms x + e in 16 bits (x = 32767 with e = 1 wraps to -32768), which the model repeats: such a row is vetoed
either way.
"""
from collections import namedtuple

import numpy as np

import kernel_census as kc

# The compared constants.  The functions read them when they are called, so that tests/test_dist_prep_model.py can move each by
# one step and show that a crafted input is then decided differently.
I8_CLAMP = 127       # the byte operand is clip(c, -127, 127)
I8_RES_MAX = 127     # a residual beyond this vetoes the byte path
I8_ROW_SLOTS = 16    # entries a row may own before it vetoes the byte path
I8_ROW_SLOTS_FULL_VETOES = False  # True: `>=` for `>` on the row slots
I8_ROW_ENT_MAX = 256  # entries the prepass collects per row
I8_LOOP_FROM = 1     # the epilogue's further-entries loops start at the row's second entry (the first has a fast path)
SLACK_ROW, SLACK_COL, SLACK_D = 1016, 508, 1  # phase-0 slack: 2|S| + 1016 B_i, 2|S| + 508 B_j + D + 64
CEN_MAX = 2048       # centred f16: |c| up to here
F16_MAX = 2048       # raw f16 (decide_kernel): integers up to here are exact in f16
WINDOW = 1 << 48     # sum r^2 * sum q^2 <= 2^48  =>  sum |r||q| <= 2^24: one f32 window is exact
WINDOW_STRICT = False  # True: `<` for `<=` at WINDOW
BK = 64              # K-step of the f16 kernels: K is padded to whole steps
N_CHUNK_CAND = 8     # prep_kernel measures windows of 64 << c dims, c = 0..7
MASH, CONTAINMENT, MAX_CONTAINMENT = 0, 1, 2

I8Rows = namedtuple("I8Rows", "e mixed c c16 a b S info n bsum slot bits ents wrap")
CenRows = namedtuple("CenRows", "fail info sumsq")
RawStats = namedtuple("RawStats", "maxabs row w2048 w1024 chunks win")
PairTerms = namedtuple("PairTerms", "G uncorrected corr_r corr_q exact slack_row slack_col")


def _i64(x):
    x = np.asarray(x)
    assert x.dtype == np.int16 and x.ndim == 2, "i16 matrices"
    return x.astype(np.int64)


# ---- centred byte operands ----------------------------------------------------------------------------------------------
def i8_rows(hv):
    """per row of an i16 matrix what prep_i8_kernel derives.  n = clamped entries, bsum = sum |b| as the kernel forms it (from
    the stored byte; None beyond I8_ROW_ENT_MAX entries, where the kernel sums whichever 256 it collected), slot = the slot
    word (None likewise), bits = the row's failure bits, ents = the row's {(d, b)}"""
    x = _i64(hv)
    e = x[:, 0] & 1
    mixed = ((x ^ x[:, :1]) & 1).any(1)
    c = (x + e[:, None]) >> 1                                     # the true centred value
    c16 = ((((x + e[:, None]) + 32768) & 0xFFFF) - 32768) >> 1    # ... as the kernel's 16-bit add gives it
    wrap = (c != c16).any(1)
    a = np.clip(c16, -I8_CLAMP, I8_CLAMP)
    b = c16 - a
    S = c16.sum(1)
    n = (b != 0).sum(1)
    b8 = ((b + 128) & 0xFF) - 128                                 # the entry's byte
    bs = np.abs(b8).sum(1)
    bsum = [int(v) if k <= I8_ROW_ENT_MAX else None for v, k in zip(bs, n)]
    n_st = np.minimum(n, I8_ROW_SLOTS)
    slot = [None if s is None else (0 if k == 0 else int(((k & 255) << 14) | (s & 0x3FFF))) for s, k in zip(bsum, n_st)]
    full = n >= I8_ROW_SLOTS if I8_ROW_SLOTS_FULL_VETOES else n > I8_ROW_SLOTS
    bits = mixed * 1 + (full | np.array([s is None or s >= 1 << 14 for s in bsum])) * 2 + (np.abs(b) > I8_RES_MAX).any(1) * 4
    ents = [{(int(d), int(b[i, d])) for d in np.nonzero(b[i])[0]} for i in range(x.shape[0])]
    return I8Rows(e, mixed, c, c16, a, b, S, 2 * S + e, n, bsum, slot, bits.astype(np.int64), ents, wrap)


def ent_word(d, b):
    """an entry as I8RowMeta.ent holds it"""
    return int(d) | ((int(b) & 0xFF) << 16)


def i8_flag(*sides):
    """the call's failure word: the OR of its rows' bits (sides: I8Rows)"""
    f = 0
    for s in sides:
        f |= int(np.bitwise_or.reduce(s.bits)) if len(s.bits) else 0
    return f


def i8_ok(hv_d, *sides):
    """the call's verdict: byte operands exist for hv_d <= 8192, hv_d % 8 == 0, and no row may fail"""
    return hv_d <= 8192 and hv_d % 8 == 0 and i8_flag(*sides) == 0


def pair_terms(mr, i, mq, j, hv_d):
    """the identity's terms for reference row i (mr: I8Rows) and query row j (mq), and the phase-0 slack of row and column"""
    G = int((mr.a[i] * mq.a[j]).sum())
    er, eq = int(mr.e[i]), int(mq.e[j])
    unc = 4 * G - 2 * eq * int(mr.S[i]) - 2 * er * int(mq.S[j]) + hv_d * er * eq
    corr_r = int((mr.b[i] * mq.c16[j]).sum())
    corr_q = int((mr.a[i] * mq.b[j]).sum())
    Bi, Bj = int(np.abs(mr.b[i]).sum()), int(np.abs(mq.b[j]).sum())
    return PairTerms(G, unc, corr_r, corr_q, unc + 4 * (corr_r + corr_q), 2 * abs(int(mr.S[i])) + SLACK_ROW * Bi,
                     2 * abs(int(mq.S[j])) + SLACK_COL * Bj + SLACK_D * hv_d + 64)


def epilogue_dot(mr, i, mq, j, hv_d):
    """the pair's dot product as the epilogue's exact phase forms it from what the prepass stored: the GEMM of the operand BYTES,
    every stored entry's byte times the other side's value -- b_r c_q with the query's true centred count, a_r b_q with the
    reference's operand byte --, a row's first entry on the fast path and its further ones in a loop from I8_LOOP_FROM, then the
    parity terms.  It equals the exact dot whenever the call is not vetoed; with a clamp, a residual limit or a loop start moved
    by one it does not.  (The device stores a row's entries in no fixed order; here they are taken by dimension.)"""
    def byte(v):
        return ((np.asarray(v, np.int64) + 128) & 0xFF) - 128
    ar, aq = byte(mr.a[i]), byte(mq.a[j])
    G = int((ar * aq).sum())
    for ents, other in ((sorted(mr.ents[i]), mq.c[j]), (sorted(mq.ents[j]), ar)):
        for t, (d, b) in enumerate(ents[:I8_ROW_SLOTS]):
            if t == 0 or t >= I8_LOOP_FROM:
                G += int(byte(b)) * int(other[d])
    er, eq = int(mr.e[i]), int(mq.e[j])
    return 4 * G - 2 * eq * int(mr.S[i]) - 2 * er * int(mq.S[j]) + hv_d * er * eq


def uncorrected_dots(mr, mq, hv_d):
    """R x Q: what the byte GEMM and the info words give without the clamped entries' corrections"""
    G = mr.a @ mq.a.T
    return 4 * G - 2 * mq.e[None, :] * mr.S[:, None] - 2 * mr.e[:, None] * mq.S[None, :] + hv_d * mr.e[:, None] * mq.e[None, :]


def correction_dots(mr, mq):
    """R x Q: 4 (sum b_r c_q + sum a_r b_q)"""
    return 4 * (mr.b @ mq.c16.T + mr.a @ mq.b.T)


def slack(mr, mq, hv_d):
    """R x Q: the phase-0 slack 2|S_r| + 1016 B_i + 2|S_q| + 508 B_j + D + 64"""
    Bi, Bj = np.abs(mr.b).sum(1), np.abs(mq.b).sum(1)
    return (2 * np.abs(mr.S) + SLACK_ROW * Bi)[:, None] + (2 * np.abs(mq.S) + SLACK_COL * Bj + SLACK_D * hv_d + 64)[None, :]


# ---- centred f16 operands -----------------------------------------------------------------------------------------------
def cen_rows(hv):
    """prep_cen_kernel: the row's fail flag (mixed parity, or |c| > 2048), info word 2 S + e and sum c^2"""
    x = _i64(hv)
    e = x[:, 0] & 1
    c = (x + e[:, None]) >> 1
    fail = ((x ^ x[:, :1]) & 1).any(1) | (np.abs(c) > CEN_MAX).any(1)
    return CenRows(fail, 2 * c.sum(1) + e, (c * c).sum(1))


def window_safe(sa, sb):
    return int(sa) * int(sb) < WINDOW if WINDOW_STRICT else int(sa) * int(sb) <= WINDOW


def cen_ok(hv_d, cr_, cq_):
    """decide_cen_kernel: no row failed and the maximum row sums of c^2 prove one window exact"""
    return hv_d % 8 == 0 and not cr_.fail.any() and not cq_.fail.any() and window_safe(cr_.sumsq.max(), cq_.sumsq.max())


# ---- raw f16 operands ---------------------------------------------------------------------------------------------------
def padded_k(hv_d):
    return (hv_d + BK - 1) // BK * BK


def raw_stats(hv):
    """prep_fast_kernel / prep_kernel: max |x|, the maximum whole-row, 2 048-window and 1 024-window sums of squares (None where
    the fast prepass does not collect window statistics: K not a multiple of 1 024, below 2 048 or beyond 32 windows) and,
    per c, the maximum over aligned chunks of 64 << c dims"""
    x = _i64(hv)
    kp = padded_k(x.shape[1])
    sq = np.zeros((x.shape[0], kp), np.int64)
    sq[:, : x.shape[1]] = x * x
    win = kp % 1024 == 0 and kp // 1024 <= 32 and kp >= 2048
    chunks = []
    for c in range(N_CHUNK_CAND):
        w = 64 << c
        pad = (kp + w - 1) // w * w
        s = np.zeros((x.shape[0], pad), np.int64)
        s[:, :kp] = sq
        chunks.append(int(s.reshape(x.shape[0], -1, w).sum(2).max()))
    w1 = int(sq.reshape(x.shape[0], -1, 1024).sum(2).max()) if win else None
    if win:  # aligned pairs of 1 024-windows; an odd last window stands alone
        t = sq.reshape(x.shape[0], -1, 1024).sum(2)
        if t.shape[1] % 2:
            t = np.concatenate([t, np.zeros((t.shape[0], 1), np.int64)], 1)
        w2 = int(t.reshape(t.shape[0], -1, 2).sum(2).max())
    else:
        w2 = None
    return RawStats(int(np.abs(x).max()), int(sq.sum(1).max()), w2, w1, chunks, win)


def raw_verdict(sr, sq_):
    """decide_kernel: 'int' when some |x| > 2048, else 0 (one window covers K), 1 / 2 (windows of 2 048 / 1 024 dims prove
    exact) or 3 (none of these)"""
    if sr.maxabs > F16_MAX or sq_.maxabs > F16_MAX:
        return "int"
    if window_safe(sr.row, sq_.row):
        return 0
    if sr.win and window_safe(sr.w2048, sq_.w2048):
        return 1
    if sr.win and window_safe(sr.w1024, sq_.w1024):
        return 2
    return 3


def raw_plan(r, q, thresholded):
    """(path, chunked) of the raw-value chain: path 0 with one window (chunked False) or several, or path 2 (the integer
    kernel, chunked None).  thresholded: the speculative schedule of hg_dist; else hg_dist_full's host-side choice"""
    sr, sq_ = raw_stats(r), raw_stats(q)
    kp = padded_k(np.asarray(r).shape[1])
    v = raw_verdict(sr, sq_)
    if v == "int":
        return 2, None

    def table():  # prep_kernel: the largest safe candidate window
        for c in range(N_CHUNK_CAND - 1, -1, -1):
            if window_safe(sr.chunks[c], sq_.chunks[c]):
                return c
        return None
    if kp <= 64 << (N_CHUNK_CAND - 1):  # some candidate covers K: the fast prepass runs
        if v == 0:
            return 0, False
        if thresholded and v in (1, 2) and kp > 2048:
            return 0, True  # the guarded windowed launch
        bc = 5 if v == 1 else 4 if v == 2 else table()
    else:
        bc = table()
    if bc is None:
        return 2, None
    return 0, (64 << bc) < kp


# ---- the call: path and kernel ------------------------------------------------------------------------------------------
def expect_dist(r, q, dist_path, dist_tile, metric=MASH, entry="dist"):
    """(hg_ctx_last_dist_path, hg_ctx_last_kernel("dist")) of a small call (R * Q < 2^24, more than 16 rows on both sides)
    under the debug keys dist_path = "i8" / "cen" / "f16" and dist_tile = "big" / "wide" / "small".  Paths: 1 = byte operands,
    3 = centred f16, 0 = raw f16, 2 = the integer kernel."""
    hv_d = np.asarray(r).shape[1]
    ctm = metric != MASH
    nt = 5 if dist_tile == "wide" else 4
    if entry == "dist" and dist_path == "i8" and i8_ok(hv_d, i8_rows(r), i8_rows(q)):
        return 1, kc.mfma_name(False, False, True, True, 4 if ctm else nt, i8=True, ctm=ctm)
    if entry == "dist" and dist_path == "cen" and cen_ok(hv_d, cen_rows(r), cen_rows(q)):
        return 3, kc.mfma_name(False, False, True, True, nt, cen=True, ctm=ctm)
    path, chunked = raw_plan(r, q, entry == "dist")
    if path == 2:
        return 2, "dist_int_kernel"
    if entry == "dist_full":
        return 0, kc.mfma_name(chunked, True, False, False, 4, ctm=ctm)
    if dist_tile == "small":
        return 0, kc.mfma_name(chunked, False, False, False, 4, ctm=ctm)
    return 0, kc.mfma_name(chunked, False, True, True, 3 if chunked else nt, ctm=ctm)
