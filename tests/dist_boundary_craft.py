"""Crafted inputs that put every exactness decision of the dist path on its constant (tests/test_gpu_dist_boundaries.py runs
them on the device, tests/test_dist_prep_model.py proves on the host that each has the property its device test relies on).

Rows are sketch-like: a family shares a parent's hashes, hv = 2 * count - n, so that every pair has a positive dot product and
an ANI strictly between 0 and 100 -- a wrong integer shows in the float.  Boundary values are then planted as centred counts
c (x = 2 c - e keeps the row's parity) at the rows and dimensions where kernels go wrong: the first rows, both sides of the
256-row tile edge, the last row; the first and last dimension, both sides of an 8-element load and of a 512-dim chunk.
"""
from collections import namedtuple

import numpy as np

Case = namedtuple("Case", "name r q sym")  # q None: one buffer compared with itself; sym: hg_dist's symmetric flag

R, Q = 301, 263          # not multiples of 4 or of a tile; both straddle row 256
RD, QD = 301, 333        # section d: Q also straddles column 320 (the wide tile)
HV_DS = (512, 4056, 4096, 8192)


def brows(n):
    return [0, 3, 4, 255, 256, n - 1]


def bdims(hv_d):
    return [0, 7, 8, 511, 512, hv_d - 1] if hv_d > 512 else [0, 7, 8, 255, 256, hv_d - 1]


def family(n, hv_d, shared, own, seed):
    """n rows of shared + own hashes each, `shared` of them the family's; parity e = (shared + own) & 1"""
    rng = np.random.default_rng(seed)
    parent = 2 * rng.binomial(shared, 0.5, hv_d) - shared
    return (parent[None, :] + 2 * rng.binomial(own, 0.5, (n, hv_d)) - own).astype(np.int16)


def two_sets(hv_d, er, eq, seed, r=R, q=Q, shared=300, own=100):
    """a reference and a query set of one family (rows of shared + own (+ e) hashes: |c| stays far below 127)"""
    hv = family(r + q, hv_d, shared, own, seed)
    rr, qq = hv[:r].copy(), hv[r:].copy()
    rr -= np.int16(er)  # one more hash with a -1 everywhere would do the same: parity e, values still sketch-like
    qq -= np.int16(eq)
    return rr, qq


def set_c(hv, row, d, c):
    """plant the centred count c at (row, d): x = 2 c - e"""
    e = int(hv[row, 0]) & 1
    hv[row, d] = 2 * c - e


# ---- a. clamp and residual ----------------------------------------------------------------------------------------------
CLAMP_OK = (127, -127, 128, -128, 254, -254)


def clamp_cases(hv_d, e):
    """byte-exact values on every boundary row and dimension (ref, qry, both), each followed by calls that plant one +-255"""
    out = []
    dims = bdims(hv_d)
    k = 0
    for side in ("ref", "qry", "both"):
        r, q = two_sets(hv_d, e, e, 100 + hv_d + e)
        for hv, on in ((r, side in ("ref", "both")), (q, side in ("qry", "both"))):
            if on:
                for t, row in enumerate(brows(len(hv))):
                    for u, d in enumerate(dims):
                        set_c(hv, row, d, CLAMP_OK[(t + u) % 6])
        out.append(Case("clamp-ok-%s" % side, r, q, False))
        for c in (255, -255):
            r2, q2 = r.copy(), q.copy()
            if side in ("ref", "both"):
                set_c(r2, brows(R)[k % 6], dims[(k // 2) % 6], c)
            if side in ("qry", "both"):
                set_c(q2, brows(Q)[(k + 1) % 6], dims[(k // 2 + 3) % 6], c)
            k += 1
            out.append(Case("clamp-veto-%s-%d" % (side, c), r2, q2, False))
    return out


def wrap_cases():
    """x + e wraps in 16 bits (32767 with e = 1), the most negative value, a row whose only odd element is x[0]"""
    out = []
    r, q = two_sets(4096, 1, 1, 140)
    r[255, 511] = 32767
    out.append(Case("wrap-32767-e1", r, q, False))
    r, q = two_sets(4096, 0, 0, 141)
    q[256, 8] = -32768
    out.append(Case("min-32768-e0", r, q, False))
    r, q = two_sets(4096, 0, 0, 142)
    r[3, 0] += 1
    out.append(Case("odd-x0-only", r, q, False))
    return out


# ---- b. entries per row -------------------------------------------------------------------------------------------------
def plant_entries(hv, row, n, seed, sign=None, dims=None):
    """n clamped entries in one row: residuals 1..127 of both signs (or `sign`), at the boundary dimensions first"""
    hv_d = hv.shape[1]
    rng = np.random.default_rng(seed)
    if dims is None:
        first = bdims(hv_d)
        rest = rng.permutation(np.setdiff1d(np.arange(hv_d), first))
        dims = (first + rest.tolist())[:n] if n < hv_d else list(range(hv_d))
    for t, d in enumerate(dims[:n]):
        s = sign if sign is not None else (1 if t % 2 == 0 else -1)
        set_c(hv, row, d, s * (128 + (t * 37) % 127))
    return list(dims[:n])


ENTRY_COUNTS_OK = (0, 1, 2, 15, 16, 16)
ENTRY_COUNTS_VETO = (17, 255, 256, 257, 4096)


def entries_cases():
    out = []
    for name, counts in (("one", (1,) * 6), ("upto16", ENTRY_COUNTS_OK)):
        r, q = two_sets(4096, 0, 1, 200)
        for t in range(6):
            plant_entries(r, brows(R)[t], counts[t], 210 + t)
            plant_entries(q, brows(Q)[t], counts[5 - t], 220 + t)
        out.append(Case("entries-%s-two" % name, r, q, False))
        out.append(Case("entries-%s-same" % name, r, None, False))
        out.append(Case("entries-%s-sym" % name, r, None, True))
    for t, n in enumerate(ENTRY_COUNTS_VETO):
        r, q = two_sets(4096, 1, 0, 230 + t)
        plant_entries(r if t % 2 == 0 else q, brows(R if t % 2 == 0 else Q)[t], n, 240 + t)
        out.append(Case("entries-veto-%d-two" % n, r, q, False))
        if t % 2 == 0:
            out.append(Case("entries-veto-%d-same" % n, r, None, False))
    return out


# ---- c. coinciding entries ----------------------------------------------------------------------------------------------
COINCIDE = (1, 2, 8, 15, 16, 16)


def coincide_cases():
    """row i and column j clamped at the same dimensions, equal and opposite signs; the diagonal of a self-comparison"""
    out = []
    rng = np.random.default_rng(300)
    dims = bdims(4096) + rng.permutation(np.setdiff1d(np.arange(4096), bdims(4096)))[:10].tolist()
    for name, sq in (("equal", 1), ("opposite", -1)):
        r, q = two_sets(4096, 1, 0, 301)
        for t in range(6):
            plant_entries(r, brows(R)[t], COINCIDE[t], 0, sign=1, dims=dims)
            plant_entries(q, brows(Q)[t], COINCIDE[5 - t], 0, sign=sq, dims=dims)
        out.append(Case("coincide-%s-two" % name, r, q, False))
    out.append(Case("coincide-self", r, None, False))
    out.append(Case("coincide-self-sym", r, None, True))
    return out


# ---- d. hits decided by the corrections ---------------------------------------------------------------------------------
RP = (0, 3, 4, 100, 255, 256, 257, 300)       # reference rows with +254 at the 16 dimensions
QP = (0, 5, 130, 255, 256, 319, 320, 332)     # query rows with +254 there: corrections at their bound, upwards
QM = (1, 6, 131, 254, 257, 318, 321, 331)     # query rows with -254 there: ... downwards
DIMS16 = (0, 7, 8, 511, 512, 1023, 1024, 2047, 2048, 2500, 3000, 3071, 3072, 3583, 3584, 4095)


def _zero_S(hv, row):
    """move the row's S = sum c to 0 in steps of one count at dimensions that are far from the clamp"""
    e = int(hv[row, 0]) & 1
    c = (hv[row].astype(np.int64) + e) >> 1
    S = int(c.sum())
    free = np.setdiff1d(np.nonzero(np.abs(c) < 100)[0], DIMS16)
    step = -1 if S > 0 else 1
    for t in range(abs(S)):
        hv[row, free[t % free.size]] += 2 * step


def decided_sets(er, eq):
    """D = 4096, rows of 3 000 hashes (2 400 shared); x = 2 * 254 - e planted at 16 common dimensions"""
    r, q = two_sets(4096, er, eq, 400, r=RD, q=QD, shared=2400, own=600)
    for hv, e in ((r, er), (q, eq)):
        np.clip(hv, -254 + e, 254 - e, out=hv)  # a handful of 4.6-sigma values: the planted entries are the only ones
    for row in RP:
        for d in DIMS16:
            set_c(r, row, d, 254)
        _zero_S(r, row)
    for rows, c in ((QP, 254), (QM, -254)):
        for row in rows:
            for d in DIMS16:
                set_c(q, row, d, c)
            _zero_S(q, row)
    return r, q


# ---- f. centred f16 -----------------------------------------------------------------------------------------------------
def flat_rows(n, hv_d, c, e, seed, flip=0.1):
    """rows whose every centred count is +-c: one sign pattern, each row flips a tenth of it; row 0 all +c, row 1 all -c"""
    rng = np.random.default_rng(seed)
    base = rng.choice(np.array([-1, 1]), hv_d)
    s = np.where(rng.random((n, hv_d)) < flip, -base[None, :], base[None, :])
    s[0], s[1] = 1, -1
    return (2 * c * s - e).astype(np.int16)


def cen_cases():
    out = []
    for e in (0, 1):
        for c in (2048, -2048, 2049, -2049):
            r, q = two_sets(4096, e, e, 500 + e)
            t = (abs(c) + e + (c < 0)) % 6
            set_c(r if c > 0 else q, brows(R if c > 0 else Q)[t], bdims(4096)[t], c)
            out.append(Case("cen-%d-e%d" % (c, e), r, q, False))
        r, q = flat_rows(R, 4096, 64, e, 510), flat_rows(Q, 4096, 64, e, 511)
        out.append(Case("cen-flat64-e%d" % e, r, q, False))
        r2 = r.copy()
        set_c(r2, 256, 4095, 65)
        out.append(Case("cen-flat64-r65-e%d" % e, r2, q, False))
        q2 = q.copy()
        set_c(q2, 3, 0, -65)
        out.append(Case("cen-flat64-q65-e%d" % e, r, q2, False))
    r, q = two_sets(4096, 0, 0, 520)
    r[4, 0] += 1
    out.append(Case("cen-mixed-first", r, q, False))
    r, q = two_sets(4096, 1, 1, 521)
    q[Q - 1, 4095] += 1
    out.append(Case("cen-mixed-last", r, q, False))
    return out


# ---- g. raw f16 chain ---------------------------------------------------------------------------------------------------
def flat_x(n, hv_d, x, seed):
    return flat_rows(n, hv_d, x, 0, seed) // 2  # every |value| = x


def raw_cases():
    """name -> Case; the verdict each must get is asserted on the host (test_dist_prep_model.py)"""
    out = []
    r, q = two_sets(4096, 0, 1, 600)
    r[255, 512] = 2048
    q[Q - 1, 4095] = -2048
    out.append(Case("raw-2048", r, q, False))
    r2 = r.copy()
    r2[256, 7] = -2049
    out.append(Case("raw-2049", r2, q, False))
    a64, b64, a128, b128 = flat_x(R, 4096, 64, 610), flat_x(Q, 4096, 64, 611), flat_x(R, 4096, 128, 612), flat_x(Q, 4096, 128, 613)

    def bump(hv, row, d):
        h = hv.copy()
        h[row, d] += np.sign(h[row, d])
        return h
    out.append(Case("raw-row-at", a64, b64, False))                     # 2^24 * 2^24: verdict 0
    out.append(Case("raw-row-above", bump(a64, 4, 8), b64, False))     # verdict 1
    out.append(Case("raw-w2048-at", a128, b64, False))                 # 2^25 * 2^23: verdict 1
    out.append(Case("raw-w2048-above", a128, bump(b64, 255, 2047), False))  # verdict 2
    out.append(Case("raw-w1024-at", a128, b128, False))                # 2^24 * 2^24: verdict 2
    out.append(Case("raw-w1024-above", bump(a128, R - 1, 1024), b128, False))  # verdict 3: the rerun
    # no window statistics: K = 1 024 (below 2 048), and K beyond the fast prepass
    c1, d1 = flat_x(R, 1000, 128, 620), flat_x(Q, 1000, 128, 621)        # 1000 * 2^14 each: product 2.4e14 < 2^48
    out.append(Case("raw-d1000-whole", c1, d1, False))
    c2, d2 = flat_x(R, 1000, 256, 622), flat_x(Q, 1000, 256, 623)        # 1000 * 2^16 each: 4.3e15 > 2^48: verdict 3
    out.append(Case("raw-d1000-rerun", c2, d2, False))
    out.append(Case("raw-d32769", flat_x(40, 32769, 16, 624), flat_x(37, 32769, 16, 625), False))
    # the fast prepass's 32-bit lane sums at their largest: every |x| = 2048 at K = 8192 (row sum 2^35) against 2^13
    big = flat_x(R, 8192, 2048, 630)
    few = np.zeros((Q, 8192), np.int16)
    rng = np.random.default_rng(631)
    for j in range(Q):
        few[j, rng.choice(8192, 2, replace=False)] = 64
    out.append(Case("raw-lane-sums", big, few, False))
    few2 = few.copy()
    few2[5, np.nonzero(few[5] == 0)[0][7]] = 1  # 2^35 * (2^13 + 1): a row sum that lost its high bits would still pass for safe
    out.append(Case("raw-lane-sums-above", big, few2, False))
    return out


SLOT_ROWS = (0, 4095, 4096, 4099)


def slot_sets():
    """4 100 small reference rows and 70 queries, one of them with sum x^2 = 2^24; slot_case() puts the reference row that
    makes the whole-row product exactly 2^48 (or one above) where the prepass files it under another statistics slot"""
    r, q = two_sets(4096, 0, 0, 640, r=4100, q=70)
    q[69] = flat_x(3, 4096, 64, 641)[2]
    return r, q


def slot_row(above):
    x = flat_x(3, 4096, 64, 642)[2].copy()
    if above:
        x[4095] = 65
    return x
