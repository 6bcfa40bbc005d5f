"""The inputs and call orders of tests/test_gpu_ctx_history.py (tests/test_ctx_history_model.py proves on the host that every
input sits where its device test needs it: accepted by the byte path, vetoed by it and accepted by the centred path, vetoed by
both, rerun by the statistics).  Built from tests/dist_boundary_craft.py: sketch-like rows of one family, boundary values
planted as centred counts.
"""
import numpy as np

import dist_boundary_craft as C

HV_D = 512
B_CLAMP = 255     # the centred count that byte operands cannot hold (residual 128) and centred f16 operands can
C_CLAMP = 2049    # ... that centred f16 operands cannot hold either; its raw value 4098 takes the integer kernel


def de_bruijn_pairs(k):
    """a cyclic order of k * k symbols below k in which every ordered pair (a, b), a == b included, is adjacent exactly once
    (the de Bruijn sequence B(k, 2) from Lyndon words); closed with its first symbol: k * k + 1 calls, k * k transitions"""
    a, seq = [0] * 3, []

    def db(t, p):
        if t > 2:
            if 2 % p == 0:
                seq.extend(a[1:p + 1])
            return
        a[t] = a[t - p]
        db(t + 1, p)
        for j in range(a[t - p] + 1, k):
            a[t] = j
            db(t + 1, t)
    db(1, 1)
    return seq + seq[:1]


def pairs_of(order):
    return {(a, b) for a, b in zip(order, order[1:])}


# ---- section a: the result block, R = 300, Q = 333 ----------------------------------------------------------------------
A_R, A_Q = 300, 333
A_KINDS = ("dist", "dist_capacity", "dist_i8_veto", "dist_cen_veto", "dist_rerun", "ham_popc", "ham_mfma", "ham_fp4", "pairs",
           "pairs_invalid", "ops", "ops_veto")
# (the issue's eleven kinds; prepared operands accepted and vetoed are two of them, which makes twelve distinct calls: the
# walk covers all 144 ordered pairs, the 121 among them)


def a_inputs():
    """name -> (r, q): plain (accepted everywhere), one +-B_CLAMP (vetoed by i8), one -C_CLAMP (vetoed by cen), and flat rows of
    |x| = 256 whose whole-row product 2^50 the speculative schedule cannot cover at K = 512 (the statistics rerun)"""
    r, q = C.two_sets(HV_D, 0, 0, 910, r=A_R, q=A_Q)
    r8, q8 = r.copy(), q.copy()
    C.set_c(r8, 256, HV_D - 1, B_CLAMP)
    C.set_c(q8, 320, 0, -B_CLAMP)
    qc = q.copy()
    C.set_c(qc, 332, 8, -C_CLAMP)
    return {"plain": (r, q), "i8_veto": (r8, q8), "cen_veto": (r, qc), "rerun": (C.flat_x(A_R, HV_D, 256, 911), C.flat_x(A_Q, HV_D, 256, 912))}


def a_pair_list(seed=913, n=500):
    rng = np.random.default_rng(seed)
    return np.stack([rng.integers(0, A_R, n), rng.integers(0, A_Q, n)], 1)


# ---- section b: padding caches ------------------------------------------------------------------------------------------
B_FILL = 1000                                  # rows of the call that fills the workspaces
B_WALK = (300, 290, 300, 511, 512, 513, 300)   # R with Q = B_Q, then Q (333 for 300) with R = 300
B_Q = 333
B_HAM = (400, 350)
B_BIG = {"i8": 254, "cen": 2000, "f16": 1024}  # centred counts planted in every row: the largest each path accepts with room
B_PLANTS = {"i8": 8, "cen": 2, "f16": 2}       # (254: residual 127; 2000 and x = 2048: two per row keep one f32 window exact)


def b_sets(path):
    """B_FILL reference and B_FILL query rows of one family with B_PLANTS[path] entries of +-B_BIG[path] in every row: a row
    that a later, smaller call leaves behind as padding holds values near the path's limit"""
    r, q = C.two_sets(HV_D, 0, 0, 930 + list(B_BIG).index(path), r=B_FILL, q=B_FILL)
    rng = np.random.default_rng(940 + list(B_BIG).index(path))
    for hv in (r, q):
        for row in range(B_FILL):
            for t, d in enumerate(rng.choice(HV_D, B_PLANTS[path], replace=False)):
                C.set_c(hv, row, int(d), B_BIG[path] if (row + t) % 2 == 0 else -B_BIG[path])
    return r, q


def b_geometries():
    """(R, Q, same) in the order the section runs them behind the filling call, up to the Hamming call"""
    out = [(R, B_Q, False) for R in B_WALK] + [(300, B_Q if Q == 300 else Q, False) for Q in B_WALK]
    return out + [(300, 300, True), (300, B_Q, False)]


# ---- section c: path memory, R * Q = 2^24 -------------------------------------------------------------------------------
PM_R, PM_Q = 8192, 2048
PM_ROW = 4099      # the reference row that B and C change
SMALL_R, SMALL_Q = 300, 333


def pm_inputs():
    """A (accepted by i8), and the one row of the reference set that makes it B (vetoed by i8, accepted by cen: +-B_CLAMP) or C
    (vetoed by both: C_CLAMP): (r, q, row of B, row of C)"""
    r, q = C.two_sets(HV_D, 0, 0, 900, r=PM_R, q=PM_Q)
    rb = r[PM_ROW:PM_ROW + 1].copy()
    C.set_c(rb, 0, 255, B_CLAMP)
    C.set_c(rb, 0, 8, -B_CLAMP)
    rc = r[PM_ROW:PM_ROW + 1].copy()
    C.set_c(rc, 0, 255, C_CLAMP)
    return r, q, rb[0], rc[0]


def pm_with(r, row):
    out = r.copy()
    out[PM_ROW] = row
    return out


def small_sets():
    return C.two_sets(HV_D, 0, 0, 901, r=SMALL_R, q=SMALL_Q)


# ---- section d: tile tables ---------------------------------------------------------------------------------------------
D_RS, D_QS = (261, 517, 773), (327, 647, 967)
D_OFFSETS = ((0, 0), (256, 0), (0, 256), (1000, 1000), (0, 1))
D_SYM_N = 700      # 3 x 3 tiles at 256 and at 320 columns: the same tile counts, but the triangle leaves out other tiles


def d_sets():
    return C.two_sets(HV_D, 0, 0, 920, r=D_RS[-1], q=D_QS[-1])
