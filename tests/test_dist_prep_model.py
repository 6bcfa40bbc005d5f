"""Host-side checks behind tests/test_gpu_dist_boundaries.py, no GPU:
  * tests/dist_prep_model.py against plain Python loops on random and hand-written rows, and its identity
    dot = uncorrected + corrections against the int64 dot product;
  * every crafted input of tests/dist_boundary_craft.py has the property its device test relies on -- exactly 16 entries, a
    residual of exactly 127 / 128, a product of exactly 2^48, uncorrected ANI < threshold <= exact ANI, ... -- so that a device
    test which would pass vacuously fails here first.
"""
import contextlib

import numpy as np
import pytest

import containment_ref as cr
import dist_boundary_craft as C
import dist_prep_model as M
import kernel_census as kc


# ---- 1. the model against loops -----------------------------------------------------------------------------------------
def loop_i8_row(x):
    e = x[0] & 1
    mixed, S, ents, bits = False, 0, [], 0
    a = []
    for d, v in enumerate(x):
        if (v ^ x[0]) & 1:
            mixed = True
        s = v + e
        if s > 32767:
            s -= 65536  # the 16-bit add
        c = s >> 1
        S += c
        ai = max(-127, min(127, c))
        a.append(ai)
        if c != ai:
            ents.append((d, c - ai))
            if abs(c - ai) > 127:
                bits |= 4
    if mixed:
        bits |= 1
    bs = sum(abs(((b + 128) & 0xFF) - 128) for _, b in ents)
    if len(ents) > 16 or bs >= 1 << 14:
        bits |= 2
    n_st = min(len(ents), 16)
    slot = ((n_st & 255) << 14 | (bs & 0x3FFF)) if n_st else 0
    return e, mixed, a, S, ents, bs, slot, bits


def hand_rows():
    rows = [
        [0] * 32, [1] * 32, [-1] * 32, [254] * 32, [256] + [0] * 31, [-254, -256] + [0] * 30, [508, 510, -508, -510] + [2] * 28,
        [507, 509, -509, -511] + [1] * 28, [32767] + [1] * 31, [-32768] + [0] * 31, [3] + [2] * 31, [2] * 31 + [3],
        [253, 255, 257, -253, -255, -257] + [7] * 26, list(range(200, 264, 2)), [-32767] * 32, [32766] * 32,
    ]
    return np.array(rows, np.int16)


def test_i8_model_equals_loops():
    rng = np.random.default_rng(1)
    rand = (2 * rng.integers(-300, 300, (40, 32)) - rng.integers(0, 2, (40, 1))).astype(np.int16)
    rand[::5, 3] += 1  # some rows of mixed parity
    for hv in (hand_rows(), rand):
        m = M.i8_rows(hv)
        for i, x in enumerate(hv.tolist()):
            e, mixed, a, S, ents, bs, slot, bits = loop_i8_row(x)
            assert (int(m.e[i]), bool(m.mixed[i]), m.a[i].tolist(), int(m.S[i]), m.ents[i], m.bsum[i], m.slot[i], int(m.bits[i])) == \
                   (e, mixed, a, S, set(ents), bs, slot, bits), (i, x)
            assert int(m.info[i]) == 2 * S + e and int(m.n[i]) == len(ents)
    m = M.i8_rows(hand_rows())
    assert m.wrap.tolist() == [i == 8 for i in range(16)]
    assert [int(b) for b in m.bits[[3, 4, 5, 6, 7, 8, 9, 10]]] == [0, 0, 0, 4, 4, 4, 4, 1]


def test_i8_identity_is_the_dot_product():
    rng = np.random.default_rng(2)
    for er in (0, 1):
        for eq in (0, 1):
            r = (2 * rng.integers(-255, 256, (12, 64)) - er).astype(np.int16)
            q = (2 * rng.integers(-255, 256, (9, 64)) - eq).astype(np.int16)
            mr, mq = M.i8_rows(r), M.i8_rows(q)
            want = r.astype(np.int64) @ q.astype(np.int64).T
            assert ((M.uncorrected_dots(mr, mq, 64) + M.correction_dots(mr, mq)) == want).all()
            for i in range(12):
                for j in range(9):
                    t = M.pair_terms(mr, i, mq, j, 64)
                    assert t.exact == want[i, j] and t.uncorrected == M.uncorrected_dots(mr, mq, 64)[i, j]
                    assert abs(t.exact - 4 * t.G) <= t.slack_row + t.slack_col - 64  # the bound the epilogue's slack rests on
                    assert M.slack(mr, mq, 64)[i, j] == t.slack_row + t.slack_col


def test_cen_and_raw_model_equal_loops():
    rng = np.random.default_rng(3)
    hv = (2 * rng.integers(-2100, 2100, (30, 2048))).astype(np.int16)
    hv[::3] = hv[::3] // 64 * 2
    hv[4, 9] += 1
    m = M.cen_rows(hv)
    for i, x in enumerate(hv.tolist()):
        e = x[0] & 1
        c = [(v + e) >> 1 for v in x]
        fail = any((v ^ x[0]) & 1 for v in x) or any(abs(v) > 2048 for v in c)
        assert (bool(m.fail[i]), int(m.info[i]), int(m.sumsq[i])) == (fail, 2 * sum(c) + e, sum(v * v for v in c)), i
    s = M.raw_stats(hv)
    sq = [[v * v for v in x] for x in hv.tolist()]
    assert s.maxabs == max(abs(v) for x in hv.tolist() for v in x) and s.row == max(sum(x) for x in sq) and s.win
    assert s.w1024 == max(sum(x[o:o + 1024]) for x in sq for o in (0, 1024)) and s.w2048 == s.row
    assert s.chunks[3] == max(sum(x[o:o + 512]) for x in sq for o in range(0, 2048, 512))
    assert not M.raw_stats(hv[:, :1000]).win and not M.raw_stats(hv[:, :1024]).win and M.raw_stats(np.zeros((1, 3072), np.int16)).win
    assert M.raw_stats(np.zeros((1, 32 * 1024), np.int16)).win and not M.raw_stats(np.zeros((1, 33 * 1024), np.int16)).win
    assert M.window_safe(1 << 24, 1 << 24) and not M.window_safe((1 << 24) + 1, 1 << 24)


# ---- 2. the crafted inputs ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("e", (0, 1))
@pytest.mark.parametrize("hv_d", C.HV_DS)
def test_clamp_cases_sit_on_127_and_254(hv_d, e):
    assert hv_d % 8 == 0 and hv_d <= 8192
    base = M.i8_rows(C.two_sets(hv_d, e, e, 100 + hv_d + e)[0])
    assert (base.n == 0).all() and (base.e == e).all() and not base.mixed.any()
    cases = C.clamp_cases(hv_d, e)
    assert [c.name.split("-")[1] for c in cases] == ["ok", "veto", "veto"] * 3
    seen_ok, seen_veto = set(), set()
    for case in cases:
        mr, mq = M.i8_rows(case.r), M.i8_rows(case.q)
        veto = "veto" in case.name
        assert M.i8_ok(hv_d, mr, mq) == (not veto), case.name
        assert M.i8_flag(mr, mq) == (4 if veto else 0)
        for m, hv, on in ((mr, case.r, "qry" not in case.name), (mq, case.q, "ref" not in case.name)):
            rows = np.nonzero(m.n)[0].tolist()
            assert rows == (C.brows(len(hv)) if on else []), case.name
            for row in rows:
                for d in C.bdims(hv_d):
                    c = int(m.c[row, d])
                    (seen_veto if abs(c) == 255 else seen_ok).add((c, d))
                    assert int(m.b[row, d]) == {127: 0, -127: 0, 128: 1, -128: -1, 254: 127, -254: -127, 255: 128, -255: -128}[c]
        path, kernel = M.expect_dist(case.r, case.q, "i8", "big")
        assert (path, kernel) == ((0, kc.mfma_name(False, False, True, True, 4)) if veto else (1, kc.mfma_name(False, False, True, True, 4, i8=True)))
    assert seen_ok == {(c, d) for c in C.CLAMP_OK for d in C.bdims(hv_d)}  # every exact value at every boundary dimension
    assert {c for c, _ in seen_veto} == {255, -255} and len({d for _, d in seen_veto}) >= 4


def test_wrap_cases():
    w, mn, odd = C.wrap_cases()
    m = M.i8_rows(w.r)
    assert m.wrap.tolist() == [i == 255 for i in range(C.R)] and int(m.bits[255]) == 4 and int(m.c16[255, 511]) == -16384
    assert M.expect_dist(w.r, w.q, "i8", "big") == (2, "dist_int_kernel")
    m = M.i8_rows(mn.q)
    assert int(m.bits[256]) == 4 and not m.mixed.any() and M.expect_dist(mn.r, mn.q, "i8", "big") == (2, "dist_int_kernel")
    m = M.i8_rows(odd.r)
    assert m.bits.tolist() == [int(i == 3) for i in range(C.R)] and (odd.r[3, 1:] % 2 == 0).all() and odd.r[3, 0] % 2 == 1
    assert M.expect_dist(odd.r, odd.q, "i8", "big")[0] == 0


def test_entries_cases_have_the_stated_counts():
    cases = {c.name: c for c in C.entries_cases()}
    for name, counts in (("one", (1,) * 6), ("upto16", C.ENTRY_COUNTS_OK)):
        c = cases["entries-%s-two" % name]
        mr, mq = M.i8_rows(c.r), M.i8_rows(c.q)
        assert mr.n[C.brows(C.R)].tolist() == list(counts) and mq.n[C.brows(C.Q)].tolist() == list(counts)[::-1]
        assert mr.n.sum() == sum(counts) and M.i8_ok(4096, mr, mq) and np.abs(mr.b).max() <= 127
        assert (mr.e == 0).all() and (mq.e == 1).all()
        for form in ("same", "sym"):
            s = cases["entries-%s-%s" % (name, form)]
            assert s.q is None and s.sym == (form == "sym") and (s.r == c.r).all()
    assert max(C.ENTRY_COUNTS_OK) == M.I8_ROW_SLOTS and min(C.ENTRY_COUNTS_VETO) == M.I8_ROW_SLOTS + 1
    assert {255, 256, 257} <= set(C.ENTRY_COUNTS_VETO) and M.I8_ROW_ENT_MAX == 256
    for t, n in enumerate(C.ENTRY_COUNTS_VETO):
        c = cases["entries-veto-%d-two" % n]
        mr, mq = M.i8_rows(c.r), M.i8_rows(c.q)
        m, row = (mr, C.brows(C.R)[t]) if t % 2 == 0 else (mq, C.brows(C.Q)[t])
        assert int(m.n[row]) == n and mr.n.sum() + mq.n.sum() == n and M.i8_flag(mr, mq) == 2  # too many entries, nothing else
        assert M.expect_dist(c.r, c.q, "i8", "big")[0] == 0
    assert (cases["entries-veto-4096-two"].r[C.brows(C.R)[4]] != 0).all()


def test_coincide_cases_share_their_dimensions():
    cases = {c.name: c for c in C.coincide_cases()}
    for name, s in (("equal", 1), ("opposite", -1)):
        c = cases["coincide-%s-two" % name]
        mr, mq = M.i8_rows(c.r), M.i8_rows(c.q)
        assert M.i8_ok(4096, mr, mq) and mr.n[C.brows(C.R)].tolist() == list(C.COINCIDE) and mq.n[C.brows(C.Q)].tolist() == list(C.COINCIDE)[::-1]
        for t, i in enumerate(C.brows(C.R)):
            for u, j in enumerate(C.brows(C.Q)):
                di, dj = {d for d, _ in mr.ents[i]}, {d for d, _ in mq.ents[j]}
                assert di <= dj or dj <= di  # one row's clamped dimensions are all the other's as well
                both = sorted(di & dj)
                assert len(both) == min(C.COINCIDE[t], C.COINCIDE[5 - u])
                assert all(np.sign(mr.b[i, d]) == s * np.sign(mq.b[j, d]) for d in both)
                assert M.pair_terms(mr, i, mq, j, 4096).exact == int(c.r[i].astype(np.int64) @ c.q[j].astype(np.int64))
    assert cases["coincide-self"].q is None and cases["coincide-self-sym"].sym


@pytest.mark.parametrize("er,eq", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_decided_pairs_are_rescued_demoted_and_tight(orc, er, eq):
    r, q = C.decided_sets(er, eq)
    mr, mq = M.i8_rows(r), M.i8_rows(q)
    assert M.i8_ok(4096, mr, mq) and (mr.e == er).all() and (mq.e == eq).all()
    assert sorted(np.nonzero(mr.n)[0].tolist()) == sorted(C.RP) and sorted(np.nonzero(mq.n)[0].tolist()) == sorted(C.QP + C.QM)
    assert (mr.n[list(C.RP)] == 16).all() and (mr.S[list(C.RP)] == 0).all() and (mq.S[list(C.QP + C.QM)] == 0).all()
    exact = cr.exact_dots(r, q)
    unc = M.uncorrected_dots(mr, mq, 4096)
    corr = M.correction_dots(mr, mq)
    assert ((unc + corr) == exact).all()
    Bi, Bj = np.abs(mr.b).sum(1), np.abs(mq.b).sum(1)
    bound = 1016 * Bi[:, None] + 508 * Bj[None, :]
    P, Qp, Qm = np.array(C.RP)[:, None], np.array(C.QP)[None, :], np.array(C.QM)[None, :]
    assert (corr[P, Qp] == bound[P, Qp]).all() and (corr[P, Qp] == 3_096_768).all()  # the corrections ARE the bound
    assert (corr[P, Qm] == -bound[P, Qm]).all()
    if er and eq:  # dot - 4 G = the whole slack but its 64: row and column sums are 0, the D term is attained too
        t = M.pair_terms(mr, C.RP[0], mq, C.QP[0], 4096)
        assert t.exact - 4 * t.G == t.slack_row + t.slack_col - 64
    rn, qn = cr.norms(r), cr.norms(q)
    for metric in (cr.MASH, cr.CONTAINMENT, cr.MAX_CONTAINMENT):
        for k in (21, 255):
            a_ex = cr.ani_ref(orc, exact, rn[:, None], qn[None, :], k, metric)
            a_un = cr.ani_ref(orc, cr.wrap_i32(unc), rn[:, None], qn[None, :], k, metric)
            up = np.nextafter(a_ex, np.float32(np.inf))
            rescued = (a_un[P, Qp] < a_ex[P, Qp])                       # th = the exact ANI: uncorrected < th <= exact
            demoted = (a_ex[P, Qm] < up[P, Qm]) & (up[P, Qm] <= a_un[P, Qm])  # th = the next float: exact < th <= uncorrected
            tight = rescued & (corr[P, Qp] >= 0.99 * bound[P, Qp])
            assert rescued.sum() >= 32 and demoted.sum() >= 32 and tight.sum() >= 4, (metric, k, rescued.sum(), demoted.sum())
            assert (a_ex[P, Qp] > 0).all() and (a_ex[P, Qp] < 100).all() and (a_ex[P, Qm] > 0).all() and (a_un[P, Qm] < 100).all()
    # corners and interiors of the 256 x 256 and 256 x 320 tiles
    assert {0, 255, 256, C.RD - 1} <= set(C.RP) and {0, 255, 256, 319, 320, C.QD - 1} <= set(C.QP) and {100} <= set(C.RP) and {130} <= set(C.QP)


def test_cen_cases_sit_on_2048_and_two_to_the_48():
    cases = {c.name: c for c in C.cen_cases()}
    for e in (0, 1):
        for c in (2048, -2048, 2049, -2049):
            case = cases["cen-%d-e%d" % (c, e)]
            mr, mq = M.cen_rows(case.r), M.cen_rows(case.q)
            x = np.concatenate([case.r, case.q]).astype(np.int64)
            cc = (x + e) >> 1
            assert np.abs(cc).max() == abs(c) and (cc == c).sum() == 1 and not ((x ^ e) & 1).any()
            assert M.cen_ok(4096, mr, mq) == (abs(c) == 2048)
            path, kernel = M.expect_dist(case.r, case.q, "cen", "big")
            assert (path, kernel) == ((3, kc.mfma_name(False, False, True, True, 4, cen=True)) if abs(c) == 2048 else (2, "dist_int_kernel"))
        flat = cases["cen-flat64-e%d" % e]
        mr, mq = M.cen_rows(flat.r), M.cen_rows(flat.q)
        assert (mr.sumsq == 1 << 24).all() and (mq.sumsq == 1 << 24).all() and M.cen_ok(4096, mr, mq)
        G = ((flat.r.astype(np.int64) + e) >> 1) @ ((flat.q.astype(np.int64) + e) >> 1).T
        assert G[0, 0] == 1 << 24 and G[0, 1] == -(1 << 24) and G[1, 1] == 1 << 24 and np.abs(G).max() == 1 << 24
        for side in ("r", "q"):
            case = cases["cen-flat64-%s65-e%d" % (side, e)]
            mr, mq = M.cen_rows(case.r), M.cen_rows(case.q)
            assert max(mr.sumsq.max(), mq.sumsq.max()) == (1 << 24) + 129 and min(mr.sumsq.max(), mq.sumsq.max()) == 1 << 24
            assert not mr.fail.any() and not mq.fail.any() and not M.cen_ok(4096, mr, mq)
            assert M.expect_dist(case.r, case.q, "cen", "big")[0] == 0
    first, last = cases["cen-mixed-first"], cases["cen-mixed-last"]
    assert M.cen_rows(first.r).fail.tolist() == [i == 4 for i in range(C.R)] and first.r[4, 0] % 2 == 1
    assert M.cen_rows(last.q).fail.tolist() == [i == C.Q - 1 for i in range(C.Q)] and last.q[C.Q - 1, 4095] % 2 == 0
    assert not M.cen_ok(4096, M.cen_rows(first.r), M.cen_rows(first.q)) and not M.cen_ok(4096, M.cen_rows(last.r), M.cen_rows(last.q))


def test_raw_cases_get_their_verdicts():
    cases = {c.name: c for c in C.raw_cases()}
    chunked, whole = kc.mfma_name(True, False, True, True, 3), kc.mfma_name(False, False, True, True, 4)

    def v(name):
        c = cases[name]
        return M.raw_verdict(M.raw_stats(c.r), M.raw_stats(c.q))

    def prod(name, field):
        c = cases[name]
        return getattr(M.raw_stats(c.r), field) * getattr(M.raw_stats(c.q), field)
    assert (v("raw-2048"), v("raw-2049")) == (0, "int") and M.raw_stats(cases["raw-2048"].r).maxabs == 2048
    assert M.raw_stats(cases["raw-2048"].q).maxabs == 2048 and M.raw_stats(cases["raw-2049"].r).maxabs == 2049
    want = {"raw-row-at": 0, "raw-row-above": 1, "raw-w2048-at": 1, "raw-w2048-above": 2, "raw-w1024-at": 2, "raw-w1024-above": 3}
    assert {n: v(n) for n in want} == want
    assert prod("raw-row-at", "row") == 1 << 48 and prod("raw-w2048-at", "w2048") == 1 << 48 and prod("raw-w1024-at", "w1024") == 1 << 48
    assert 0 < prod("raw-row-above", "row") - (1 << 48) < 1 << 33 and 0 < prod("raw-w2048-above", "w2048") - (1 << 48) < 1 << 33
    assert 0 < prod("raw-w1024-above", "w1024") - (1 << 48) < 1 << 34
    for name, k in want.items():  # verdict 0: the whole-K kernel; 1, 2: the guarded windowed launch; 3: the rerun, windowed as well
        c = cases[name]
        assert M.expect_dist(c.r, c.q, "f16", "big") == (0, whole if k == 0 else chunked), name
        assert M.expect_dist(c.r, c.q, "f16", "big", entry="dist_full") == (0, kc.mfma_name(k != 0, True, False, False, 4)), name
    assert M.raw_plan(cases["raw-w1024-above"].r, cases["raw-w1024-above"].q, True) == (0, True)
    for name in ("raw-d1000-whole", "raw-d1000-rerun", "raw-d32769"):
        assert not M.raw_stats(cases[name].r).win
    assert v("raw-d1000-whole") == 0 and v("raw-d1000-rerun") == 3
    s = M.raw_stats(cases["raw-d1000-rerun"].r)
    assert s.chunks[2] ** 2 == 1 << 48 and s.chunks[3] ** 2 > 1 << 48  # the rerun's table: windows of 256 dims, at the bound
    assert M.expect_dist(cases["raw-d1000-rerun"].r, cases["raw-d1000-rerun"].q, "f16", "big") == (0, chunked)
    c = cases["raw-d32769"]
    assert M.padded_k(32769) > 8192 and M.expect_dist(c.r, c.q, "f16", "big") == (0, chunked)
    c = cases["raw-lane-sums"]  # a lane of prep_fast_kernel sums K / 64 = 128 squares of 2^22: 2^29, the most it ever holds
    sr, sq = M.raw_stats(c.r), M.raw_stats(c.q)
    assert (np.abs(c.r) == 2048).all() and sr.row == 1 << 35 and sq.row == 1 << 13 and sr.row * sq.row == 1 << 48 and v("raw-lane-sums") == 0
    assert 8192 // 64 * 2048 * 2048 < 1 << 32
    c = cases["raw-lane-sums-above"]  # one above: only the exact 2^35 gives verdict 1 (any sum that wrapped in 32 bits is smaller)
    assert M.raw_stats(c.q).row == (1 << 13) + 1 and v("raw-lane-sums-above") == 1 and M.expect_dist(c.r, c.q, "f16", "big") == (0, chunked)


def test_slot_sets_put_the_extremal_row_alone():
    r, q = C.slot_sets()
    assert r.shape == (4100, 4096) and (4095 // 4) % 1024 == 1023 and (4096 // 4) % 1024 == 0  # prep_fast_kernel: slot = (row / 4) % 1024
    sq = M.raw_stats(q)
    assert sq.row == 1 << 24 and M.raw_stats(q[:69]).row < 1 << 22 and M.raw_stats(r).row < 1 << 22
    for above in (False, True):
        for row in C.SLOT_ROWS:
            r2 = r.copy()
            r2[row] = C.slot_row(above)
            s = M.raw_stats(r2)
            assert s.row == (1 << 24) + (129 if above else 0) and M.raw_verdict(s, sq) == (1 if above else 0)


# ---- 3. the constants, each moved by one: the crafted inputs tell the difference ------------------------------------------
def phase0_bound(th, k, nr, nq):
    """the Mash-style pre-filter of hg_dist_kernels.hip in float64: a pair goes on to the exact phase iff
    4 G + slack >= pre_c * (nr + nq), pre_c from the threshold with its 1e-4 and 1e-5 safety margins"""
    x = np.exp(k * (th / 100.0 - 1.0))
    j = x / (2.0 - x) * (1.0 - 1e-4)
    return j / (1.0 + j) * (1.0 - 1e-5) * (nr + nq)


def test_epilogue_restatement_is_exact_on_the_entry_cases():
    """M.epilogue_dot -- operand bytes, stored entry bytes, first entry and further-entries loop -- gives the int64 dot product on
    every boundary row and column of the entry inputs as long as no constant is moved"""
    cases = {c.name: c for c in C.entries_cases() + C.coincide_cases() + C.clamp_cases(4096, 1)[6:7]}
    for name in ("entries-upto16-two", "entries-one-two", "coincide-equal-two", "coincide-opposite-two", "clamp-ok-both"):
        c = cases[name]
        mr, mq = M.i8_rows(c.r), M.i8_rows(c.q)
        for i in C.brows(C.R) + [10]:
            for j in C.brows(C.Q) + [10]:
                assert M.epilogue_dot(mr, i, mq, j, 4096) == int(c.r[i].astype(np.int64) @ c.q[j].astype(np.int64)), (name, i, j)


def test_every_constant_moved_by_one_changes_a_crafted_decision(orc, monkeypatch):
    """the host-side counterpart of profiles/dist_boundary_mutations.md: each compared constant of tests/dist_prep_model.py is moved
    by one step (monkeypatched, one at a time) and the model's own decision -- the phase-0 filter, i8_ok / i8_flag, the stored
    bytes and the epilogue's dot, cen_ok, raw_verdict, expect_dist -- is evaluated again on a crafted input: it must change.
    So the device test that runs this input against the unmoved model can tell the two apart."""
    @contextlib.contextmanager
    def moved(**kw):
        with monkeypatch.context() as m:
            for k, v in kw.items():
                assert getattr(M, k) != v
                m.setattr(M, k, v)
            yield

    def dot(c, i, j):
        return int(c.r[i].astype(np.int64) @ c.q[j].astype(np.int64))

    # the slack: a tight rescued pair at the threshold of its own exact ANI survives phase 0 only with the full slack
    for er, eq in ((0, 0), (1, 1)):
        r, q = C.decided_sets(er, eq)
        mr, mq = M.i8_rows(r), M.i8_rows(q)
        rn, qn = cr.norms(r).astype(np.int64), cr.norms(q).astype(np.int64)
        i, j = C.RP[3], C.QP[2]
        th = float(cr.ani_ref(orc, np.array([[M.pair_terms(mr, i, mq, j, 4096).exact]], np.int32), rn[i:i + 1, None], qn[None, j:j + 1], 21, cr.MASH)[0, 0])

        def survives():
            t = M.pair_terms(mr, i, mq, j, 4096)
            assert t.slack_row + t.slack_col == M.slack(mr, mq, 4096)[i, j]
            return 4 * t.G + t.slack_row + t.slack_col >= phase0_bound(th, 21, rn[i], qn[j])
        assert survives()
        for kw in (dict(SLACK_ROW=508), dict(SLACK_COL=254)) + ((dict(SLACK_D=0),) if er and eq else ()):
            with moved(**kw):
                assert not survives(), (kw, er, eq)
    # the row slots: `>=` vetoes a row of exactly 16 entries
    up = {c.name: c for c in C.entries_cases()}["entries-upto16-two"]
    assert M.i8_flag(M.i8_rows(up.r), M.i8_rows(up.q)) == 0 and M.expect_dist(up.r, up.q, "i8", "big")[0] == 1
    with moved(I8_ROW_SLOTS_FULL_VETOES=True):
        assert M.i8_flag(M.i8_rows(up.r), M.i8_rows(up.q)) == 2 and M.expect_dist(up.r, up.q, "i8", "big")[0] == 0
    # the further-entries loop: a row / a column of two entries, every entry's product not 0 (the device keeps no order)
    mr, mq = M.i8_rows(up.r), M.i8_rows(up.q)
    i2, j2 = C.brows(C.R)[2], C.brows(C.Q)[3]
    assert int(mr.n[i2]) == 2 and int(mq.n[j2]) == 2 and int(mr.n[10]) == 0 and int(mq.n[10]) == 0
    assert all(b * int(mq.c[10, d]) != 0 for d, b in mr.ents[i2]) and all(b * int(mr.a[10, d]) != 0 for d, b in mq.ents[j2])
    for i, j in ((i2, 10), (10, j2)):
        assert M.epilogue_dot(mr, i, mq, j, 4096) == dot(up, i, j)
        with moved(I8_LOOP_FROM=2):
            assert M.epilogue_dot(mr, i, mq, j, 4096) != dot(up, i, j)
    # the residual: one c = +-255 has b = +-128; let through, the call is not vetoed and the entry's byte is -b
    veto = C.clamp_cases(4096, 0)[1]
    i = int(np.nonzero(np.abs(M.i8_rows(veto.r).b).max(1) == 128)[0][0])
    assert M.i8_flag(M.i8_rows(veto.r), M.i8_rows(veto.q)) == 4 and M.expect_dist(veto.r, veto.q, "i8", "big")[0] == 0
    with moved(I8_RES_MAX=128):
        mr, mq = M.i8_rows(veto.r), M.i8_rows(veto.q)
        assert M.i8_flag(mr, mq) == 0 and M.expect_dist(veto.r, veto.q, "i8", "big")[0] == 1
        assert M.epilogue_dot(mr, i, mq, 10, 4096) != dot(veto, i, 10)
    # the clamp: c = +-128 stored as the byte -+128
    ok = C.clamp_cases(4096, 0)[0]
    a0 = M.i8_rows(ok.r).a
    assert M.epilogue_dot(M.i8_rows(ok.r), 0, M.i8_rows(ok.q), 10, 4096) == dot(ok, 0, 10)
    with moved(I8_CLAMP=128):
        mr, mq = M.i8_rows(ok.r), M.i8_rows(ok.q)
        assert (mr.a != a0).any() and M.i8_flag(mr, mq) == 0
        assert [M.epilogue_dot(mr, i, mq, 10, 4096) != dot(ok, i, 10) for i in C.brows(C.R)] == [True] * 6
    # 2048 in the centred prepass and in decide_kernel
    cen = {c.name: c for c in C.cen_cases()}
    for name in ("cen-2049-e0", "cen--2049-e1"):
        c = cen[name]
        assert not M.cen_ok(4096, M.cen_rows(c.r), M.cen_rows(c.q)) and M.expect_dist(c.r, c.q, "cen", "big") == (2, "dist_int_kernel")
        with moved(CEN_MAX=2049):
            assert M.cen_ok(4096, M.cen_rows(c.r), M.cen_rows(c.q)) and M.expect_dist(c.r, c.q, "cen", "big")[0] == 3
    raw = {c.name: c for c in C.raw_cases()}
    c = raw["raw-2049"]
    assert M.raw_verdict(M.raw_stats(c.r), M.raw_stats(c.q)) == "int" and M.expect_dist(c.r, c.q, "f16", "big") == (2, "dist_int_kernel")
    with moved(F16_MAX=2049):
        assert M.raw_verdict(M.raw_stats(c.r), M.raw_stats(c.q)) == 0 and M.expect_dist(c.r, c.q, "f16", "big")[0] == 0
    # 2^48: `<` turns every "at" input down, 2^49 lets every "above" input through
    def decisions(names, cens):
        out = [M.raw_verdict(M.raw_stats(raw[n].r), M.raw_stats(raw[n].q)) for n in names]
        out += [M.expect_dist(raw[n].r, raw[n].q, "f16", "big")[1] for n in names[:1]]
        out += [M.cen_ok(4096, M.cen_rows(cen[n].r), M.cen_rows(cen[n].q)) for n in cens]
        return out + [M.expect_dist(cen[n].r, cen[n].q, "cen", "big")[0] for n in cens]
    whole, chunked = kc.mfma_name(False, False, True, True, 4), kc.mfma_name(True, False, True, True, 3)
    at = (("raw-row-at", "raw-w2048-at", "raw-w1024-at"), ("cen-flat64-e0", "cen-flat64-e1"))
    above = (("raw-row-above", "raw-w2048-above", "raw-w1024-above"), ("cen-flat64-r65-e0", "cen-flat64-q65-e1"))
    assert decisions(*at) == [0, 1, 2, whole, True, True, 3, 3] and decisions(*above) == [1, 2, 3, chunked, False, False, 0, 0]
    with moved(WINDOW_STRICT=True):
        assert decisions(*at) == [1, 2, 3, chunked, False, False, 0, 0]
    with moved(WINDOW=1 << 49):
        assert decisions(*above) == [0, 1, 2, whole, True, True, 3, 3]
