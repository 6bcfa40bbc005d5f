"""Host-side checks behind tests/test_gpu_ctx_history.py, no GPU:
  * the invariants of tests/ctx_history_model.py on seeded random call lists -- a signature never survives a call on other
    operands, the countdown reaches 0 after exactly 16 calls that do not try byte operands, a rerun happens only on a trusted
    signature, hg_dist_full* leaves the signatures alone;
  * the hand-written sequences of the device file against the states they are meant to reach;
  * every crafted input of tests/ctx_history_craft.py sits where the device file needs it, so that a sequence whose inputs
    drifted fails here first instead of testing nothing.
"""
import numpy as np
import pytest

import ctx_history_craft as H
import ctx_history_model as HM
import dist_prep_model as M
import kernel_census as kc

RAW0 = (0, False)


def rand_call(rng):
    ref, qry = int(rng.integers(0, 3)), int(rng.integers(3, 6))
    large = rng.random() < 0.5
    R, Q = (8192, 2048) if large else (int(rng.integers(17, 400)), int(rng.integers(17, 400)))
    if rng.random() < 0.1:
        Q = int(rng.integers(1, 17))
    entry = ("dist", "dist", "dist", "dist_full", "ops")[int(rng.integers(0, 5))]
    return HM.call(entry, ref, qry, R, Q, 512, rng.random() < 0.5, rng.random() < 0.6, RAW0 if rng.random() < 0.8 else (2, None),
                   dist_path=("", "", "i8", "cen", "f16")[int(rng.integers(0, 5))], dist_tile=("", "big", "wide")[int(rng.integers(0, 3))],
                   metric=int(rng.integers(0, 3)))


def sig_of(c):
    return (c.ref, c.qry, c.R, c.Q, c.hv_d)


@pytest.mark.parametrize("seed", range(8))
def test_invariants_on_random_call_lists(seed):
    rng = np.random.default_rng(seed)
    st = HM.START
    since_veto = None  # calls that did not try byte operands since the last veto
    for n in range(4000):
        c = rand_call(rng)
        new, e = HM.step(st, c)
        what = (seed, n, c, st, new, e)
        # signatures: only this call's operands can be remembered behind it, at most one path, and only the path that ran
        for s in (new.i8_sig, new.cen_sig):
            assert s is None or s == sig_of(c) or (c.entry in ("dist_full", "ops") and s in (st.i8_sig, st.cen_sig)), what
        assert not (new.i8_sig and new.cen_sig) or c.entry in ("dist_full", "ops"), what
        if c.entry == "dist":
            assert (new.i8_sig == sig_of(c)) == (e.path == 1) and (new.cen_sig == sig_of(c)) == (e.path == 3), what
            assert e.path in (0, 1, 2, 3) and e.kernel, what
            assert (e.path == 1) == (e.tried_i8 and c.i8_ok), what
            assert e.path != 3 or (e.tried_cen and c.cen_ok), what
            assert not e.rerun or (sig_of(c) in (st.i8_sig, st.cen_sig) and e.path in (0, 2)), what
            assert not e.tried_i8 or st.skip == 0 or c.dist_path == "i8", what
            assert e.tried_i8 or c.dist_path == "i8" or not (HM.is_large(c) and st.skip == 0 and c.dist_path != "f16") or HM.is_skinny(c), what
        if c.entry == "dist_full":
            assert (new.i8_sig, new.cen_sig) == (st.i8_sig, st.cen_sig) and not e.tried_i8 and not e.tried_cen and e.path in (0, 2), what
        if c.entry == "ops":
            assert new.i8_sig is None and new.cen_sig == st.cen_sig and new.skip == st.skip and (e.path == 1) == c.i8_ok, what
        # the countdown
        assert 0 <= new.skip <= HM.SKIP_CALLS, what
        vetoed = c.entry == "dist" and e.tried_i8 and not c.i8_ok
        counts = c.entry == "dist_full" or (c.entry == "dist" and not e.tried_i8 and not HM.is_skinny(c))
        if vetoed:
            assert new.skip == HM.SKIP_CALLS, what
            since_veto = 0
        elif since_veto is not None:
            since_veto += counts
            assert new.skip == max(HM.SKIP_CALLS - since_veto, 0), what
            assert (new.skip == 0) == (since_veto >= HM.SKIP_CALLS), what
        st = new


def test_countdown_is_sixteen_calls():
    big_ok = HM.call("dist", 1, 2, 8192, 2048, 512, True, True, RAW0)
    big_veto = big_ok._replace(i8_ok=False)
    small = HM.call("dist", 3, 4, 300, 333, 512, True, True, RAW0)
    for n_small, want_path in ((16, 1), (15, 3), (0, 3)):
        h = HM.History()
        assert [h.step(c).path for c in (big_ok, big_ok, big_veto)] == [1, 1, 0] and h.log[-1][1].rerun and h.state.skip == 16
        for _ in range(n_small):
            assert h.step(small).path == 0
        assert h.state.skip == 16 - n_small
        e = h.step(big_ok)
        assert e.path == want_path and e.tried_i8 == (want_path == 1), (n_small, e)


def test_centred_trust_and_rerun():
    b = HM.call("dist", 1, 2, 8192, 2048, 512, False, True, RAW0)
    c = b._replace(cen_ok=False, raw_spec=(2, None), raw_host=(2, None))
    h = HM.History()
    got = [h.step(x) for x in (b, b, c, b)]
    assert [e.path for e in got] == [3, 3, 2, 3] and [e.rerun for e in got] == [False, False, True, False]
    assert [e.tried_i8 for e in got] == [True, False, False, False] and h.state.skip == 13 and h.state.cen_sig == sig_of(b)
    assert got[2].kernel == "dist_int_kernel" and got[0].kernel == kc.mfma_name(False, False, True, True, 4, cen=True)


def test_signatures_ignore_metric_and_ksize_and_follow_pointers():
    a = HM.call("dist", 1, 2, 8192, 2048, 512, True, True, RAW0)
    h = HM.History()
    for metric in (M.MASH, M.CONTAINMENT, M.MAX_CONTAINMENT, M.MASH):
        e = h.step(a._replace(metric=metric))
        assert e.path == 1 and h.state.i8_sig == sig_of(a) and ("ctm" in e.kernel) == (metric != M.MASH)
    full = a._replace(entry="dist_full")
    assert h.step(full).kernel == kc.mfma_name(False, True, False, False, 4) and h.state.i8_sig == sig_of(a)
    # three row blocks: other pointers and sizes, none of them large
    for r0, rows in HM.blocks(8192, 2048, 2731 * 2048):
        e = h.step(a._replace(ref=("blk", r0), R=rows))
        assert e.path == 0 and not e.tried_i8 and h.state.i8_sig is None
    assert HM.blocks(8192, 2048, 2731 * 2048) == [(0, 2731), (2731, 2731), (5462, 2730)]
    assert h.step(a).path == 1 and HM.hamming_mfma(h.state).i8_sig is None


def test_de_bruijn_walks_visit_every_ordered_pair():
    for k in (2, 3, 11, 12, 17):
        order = H.de_bruijn_pairs(k)
        assert len(order) == k * k + 1 and len(H.pairs_of(order)) == k * k and set(order) == set(range(k))


# ---- the crafted inputs ---------------------------------------------------------------------------------------------------
def verdicts(r, q):
    hv_d = r.shape[1]
    return (M.i8_ok(hv_d, M.i8_rows(r), M.i8_rows(q)), M.cen_ok(hv_d, M.cen_rows(r), M.cen_rows(q)), M.raw_plan(r, q, True), M.raw_plan(r, q, False))


def test_path_memory_inputs_sit_on_their_boundaries():
    r, q, rb, rc = H.pm_inputs()
    assert r.shape == (H.PM_R, H.HV_D) and q.shape == (H.PM_Q, H.HV_D) and H.PM_R * H.PM_Q == HM.LARGE
    assert verdicts(r, q) == (True, True, (0, False), (0, False))                       # A: byte operands
    assert verdicts(H.pm_with(r, rb), q) == (False, True, (0, False), (0, False))       # B: vetoed by i8, centred operands
    assert verdicts(H.pm_with(r, rc), q) == (False, False, (2, None), (2, None))        # C: vetoed by both, the integer kernel
    # B's veto is the residual alone, on the limit: one less and the byte path would take it
    mb = M.i8_rows(rb[None, :])
    assert int(mb.bits[0]) == 4 and sorted(b for _, b in mb.ents[0]) == [-128, 128] and (rb != r[H.PM_ROW]).sum() == 2
    mc = M.cen_rows(rc[None, :])
    assert bool(mc.fail[0]) and int(np.abs((rc.astype(np.int64) + (rc[0] & 1)) >> 1).max()) == M.CEN_MAX + 1
    rs, qs = H.small_sets()
    assert rs.shape[0] * qs.shape[0] < HM.LARGE and min(rs.shape[0], qs.shape[0]) > HM.SKINNY_MAX
    assert verdicts(rs, qs)[2:] == ((0, False), (0, False))


def test_result_block_inputs_sit_where_their_calls_need_them():
    s = H.a_inputs()
    assert verdicts(*s["plain"]) == (True, True, (0, False), (0, False))
    assert verdicts(*s["i8_veto"]) == (False, True, (0, False), (0, False))
    assert verdicts(*s["cen_veto"])[1:] == (False, (2, None), (2, None))
    # the rerun: no |x| beyond f16, the whole-row product beyond one window, K below the window statistics -- the speculative
    # schedule covers verdict 0 alone -- and windows of 256 dims exact
    r, q = s["rerun"]
    sr, sq = M.raw_stats(r), M.raw_stats(q)
    assert M.raw_verdict(sr, sq) == 3 and not sr.win and M.raw_plan(r, q, True) == (0, True) and sr.chunks[2] * sq.chunks[2] == M.WINDOW
    for r, q in s.values():
        assert r.shape == (H.A_R, H.HV_D) and q.shape == (H.A_Q, H.HV_D)
    ij = H.a_pair_list()
    assert ij[:, 0].max() < H.A_R and ij[:, 1].max() < H.A_Q
    assert len(H.A_KINDS) == 12 and len(H.pairs_of(H.de_bruijn_pairs(12))) == 144


def test_tile_table_grids_are_nine_and_outnumber_the_cache():
    for bn in (320, 256):
        grids = {((R + 255) // 256, (Q + bn - 1) // bn) for R in H.D_RS for Q in H.D_QS}
        assert len(grids) == 9 > 8
    r, q = H.d_sets()
    assert verdicts(r, q)[2] == (0, False)
    assert len({ro - qo for ro, qo in H.D_OFFSETS}) == 4 and sum(ro == qo for ro, qo in H.D_OFFSETS) == 2
    # the symmetric grid that only the tile width tells apart: equal tile counts, and the wide tiles need a tile the narrow
    # ones leave out (a table found by its tile counts alone would drop hits)
    n = H.D_SYM_N
    assert ((n + 255) // 256, (n + 255) // 256) == ((n + 255) // 256, (n + 319) // 320) == (3, 3)
    work = {bn: {(tm, tn) for tm in range(3) for tn in range(3) if not tm * 256 >= tn * bn + bn} for bn in (256, 320)}
    assert work[256] < work[320] and (1, 0) in work[320] - work[256]
