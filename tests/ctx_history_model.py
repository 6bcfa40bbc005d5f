"""What a context remembers about the dist path from one call to the next, restated on the host: the countdown i8_skip and
the two signatures "the previous call on exactly these operands ran on byte / on centred operands" (hg_run_dist and
dist_block_once: hg_dist_kernels.hip, hg_api_dist.hip), and what a call then reports through hg_ctx_last_dist_path and
hg_ctx_last_kernel("dist").

Pure Python on top of tests/dist_prep_model.py, whose i8_ok, cen_ok and raw_plan say what the prepasses decide about an input;
nothing here calls the library.  tests/test_ctx_history_model.py checks the model's own invariants,
tests/test_gpu_ctx_history.py checks the device against it call by call.

The rules, as the comments of the two functions give them:
  * a call tries byte operands when it is thresholded, hv_d <= 8192 and a multiple of 8, the debug key dist_path is not "f16",
    the problem is large (R * Q >= 2^24) or dist_path = "i8", and the countdown is 0 or dist_path = "i8";
  * a vetoed attempt sets the countdown to 16; every dist call that reaches the operand paths without trying byte operands --
    thresholded or full -- takes one off.  A rerun is part of its call and takes nothing off;
  * the call behind a byte-operand call on the same (pointers, R, Q, hv_d) trusts that path: no fallback is queued, and a veto
    is rerun through the statistics-driven raw-value schedule.  The same holds for centred operands, which are tried behind
    a byte attempt that was not trusted when the problem is large or dist_path = "cen";
  * a thresholded call sets the signature of the path that did its work and clears the other one; the signatures are pointers
    and sizes, neither the metric nor ksize; hg_dist_full* tries neither path and leaves both signatures alone;
  * the streaming kernel (at most 16 rows on one side, no debug key) runs in front of all this: it takes nothing off the
    countdown, and its call clears both signatures like any thresholded call that ran on neither path;
  * prepared operands (hg_dist_block_ops_dev) always try byte operands, never fall back, and clear the byte signature.
"""
from collections import namedtuple

import dist_prep_model as M
import kernel_census as kc

SKIP_CALLS = 16          # calls that skip the byte attempt after a veto
LARGE = 1 << 24          # R * Q from which byte and centred operands are tried unprompted
SKINNY_MAX = 16          # rows of the small side up to which the streaming kernel takes the call
N_CU = 256               # compute units of the device the kernel names are predicted for (tile_nt)

State = namedtuple("State", "skip i8_sig cen_sig")
START = State(0, None, None)

# One call.  entry: "dist" (hg_dist_dev / hg_dist_block_dev, one block), "dist_full" or "ops" (prepared operands);
# ref, qry: the operands' identities (device pointers, or any hashable stand-in); dist_path / dist_tile: the debug keys;
# i8_ok, cen_ok: what the prepasses decide about the contents; raw_spec / raw_host: dist_prep_model.raw_plan(r, q, True / False)
Call = namedtuple("Call", "entry ref qry R Q hv_d dist_path dist_tile metric i8_ok cen_ok raw_spec raw_host")
Expect = namedtuple("Expect", "path kernel rerun tried_i8 tried_cen")


def call(entry, ref, qry, R, Q, hv_d, i8_ok, cen_ok, raw_spec, raw_host=None, dist_path="", dist_tile="", metric=M.MASH):
    return Call(entry, ref, qry, R, Q, hv_d, dist_path, dist_tile, metric, bool(i8_ok), bool(cen_ok), raw_spec, raw_host or raw_spec)


def describe(entry, ref, qry, r, q, dist_path="", dist_tile="", metric=M.MASH):
    """the Call of the i16 matrices r and q (q may be r) held at the identities ref and qry"""
    hv_d = r.shape[1]
    same = q is r
    ir, cr_ = M.i8_rows(r), M.cen_rows(r)
    iq, cq_ = (ir, cr_) if same else (M.i8_rows(q), M.cen_rows(q))
    return call(entry, ref, qry, r.shape[0], q.shape[0], hv_d, M.i8_ok(hv_d, ir, iq), M.cen_ok(hv_d, cr_, cq_),
                M.raw_plan(r, q, True), M.raw_plan(r, q, False), dist_path, dist_tile, metric)


def tile_nt(c, num, den):
    """16-column MFMA tiles per wave of the 256-row geometries: the debug key, else the cheaper of 256 and 320 columns"""
    if c.dist_tile == "big":
        return 4
    if c.dist_tile == "wide":
        return 5
    tm = (c.R + 255) // 256
    r4 = (tm * ((c.Q + 255) // 256) + N_CU - 1) // N_CU
    r5 = (tm * ((c.Q + 319) // 320) + N_CU - 1) // N_CU
    return 5 if r5 * num < r4 * den else 4


def is_large(c):
    return c.R * c.Q >= LARGE


def is_skinny(c):
    return c.entry == "dist" and min(c.R, c.Q) <= SKINNY_MAX and c.hv_d % 8 == 0 and not c.dist_path and not c.dist_tile


def _raw(c, plan, thresholded):
    """(path, kernel) of the raw-value chain"""
    path, chunked = plan
    ctm = c.metric != M.MASH
    if path == 2:
        return 2, "dist_int_kernel"
    if not thresholded:
        return 0, kc.mfma_name(chunked, True, False, False, 4, ctm=ctm)
    fills = c.dist_tile in ("big", "wide") or (c.dist_tile != "small" and c.R * c.Q >= 256 ** 3)
    if not fills:
        return 0, kc.mfma_name(chunked, False, False, False, 4, ctm=ctm)
    return 0, kc.mfma_name(chunked, False, True, True, 3 if chunked else tile_nt(c, 5, 4), ctm=ctm)


def step(st, c):
    """(the state behind the call, what the call reports)"""
    ctm = c.metric != M.MASH
    sig = (c.ref, c.qry, c.R, c.Q, c.hv_d)
    i8_possible = c.hv_d <= 8192 and c.hv_d % 8 == 0
    if c.entry == "ops":
        assert i8_possible, "prepared operands: hv_d <= 8192, hv_d % 8 == 0"
        nt = 4 if ctm else tile_nt(c, 9, 8)
        ok = Expect(1, kc.mfma_name(False, False, True, True, nt, i8=True, ctm=ctm), False, True, False)
        return st._replace(i8_sig=None), ok if c.i8_ok else Expect(None, None, False, True, False)  # vetoed: HG_ERR_INEXACT, nothing reported
    if c.entry == "dist_full":
        path, kernel = _raw(c, c.raw_host, False)
        return st._replace(skip=max(st.skip - 1, 0)), Expect(path, kernel, False, False, False)
    assert c.entry == "dist", c.entry
    if is_skinny(c):
        return State(st.skip, None, None), Expect(2, "dist_skinny_kernel<%s>" % ("false" if c.Q <= c.R else "true"), False, False, False)
    want_i8 = c.dist_path != "f16" and i8_possible and (is_large(c) or c.dist_path == "i8") and (st.skip == 0 or c.dist_path == "i8")
    skip = st.skip if want_i8 else max(st.skip - 1, 0)
    rerun = False
    if want_i8:
        if c.i8_ok:
            nt = 4 if ctm else tile_nt(c, 9, 8)
            return State(skip, sig, None), Expect(1, kc.mfma_name(False, False, True, True, nt, i8=True, ctm=ctm), False, True, False)
        skip = SKIP_CALLS
        rerun = st.i8_sig == sig
    want_cen = not rerun and c.hv_d % 8 == 0 and c.dist_path != "f16" and (is_large(c) or c.dist_path == "cen")
    if want_cen:
        if c.cen_ok:
            return State(skip, None, sig), Expect(3, kc.mfma_name(False, False, True, True, tile_nt(c, 5, 4), cen=True, ctm=ctm), False, want_i8, True)
        rerun = st.cen_sig == sig
    path, kernel = _raw(c, c.raw_host if rerun else c.raw_spec, True)
    return State(skip, None, None), Expect(path, kernel, rerun, want_i8, want_cen)


def hamming_mfma(st):
    """a Hamming search on the matrix pipe overwrites the byte operand copies: the byte signature goes"""
    return st._replace(i8_sig=None)


def blocks(R, Q, pair_limit):
    """[(first row, rows)] of the blocks hg_dist_block_dev cuts a call of more than pair_limit pairs into (hg_run_blocks)"""
    if not pair_limit or R * Q <= pair_limit:
        return [(0, R)]
    per = max(1, pair_limit // Q)
    return [(r0, min(per, R - r0)) for r0 in range(0, R, per)]


class History:
    """the state of one context, advanced call by call"""

    def __init__(self):
        self.state = START
        self.log = []

    def step(self, c):
        self.state, e = step(self.state, c)
        self.log.append((c, e, self.state))
        return e
