"""The columns of hg_ani_pairs (include/hypergen.h: HG_PAIRS_*) restated for the tests on top of tests/containment_ref.py: the
column layout -- a pair's values in ascending order of the column bits -- and CONTAINMENT_REF, which is the containment metric
with the two norms exchanged (dot / nr: the share of the reference's hashes found in the query)."""
import numpy as np

import containment_ref as cr

MASH, CONTAINMENT, MAX_CONTAINMENT, CONTAINMENT_REF = 1, 2, 4, 8
BITS = (MASH, CONTAINMENT, MAX_CONTAINMENT, CONTAINMENT_REF)
ALL = 15
EMPTY = 0xFFFFFFFF
NAMES = {"mash": MASH, "containment": CONTAINMENT, "max_containment": MAX_CONTAINMENT, "containment_ref": CONTAINMENT_REF}
METRIC_BIT = {cr.MASH: MASH, cr.CONTAINMENT: CONTAINMENT, cr.MAX_CONTAINMENT: MAX_CONTAINMENT}  # ctx metric -> its column


def column(orc, bit, dot, nr, nq, k):
    """float32 values of one column for arrays of (dot, nr, nq)"""
    if bit == CONTAINMENT_REF:
        return cr.ani_ref(orc, dot, nq, nr, k, cr.CONTAINMENT)
    return cr.ani_ref(orc, dot, nr, nq, k, {MASH: cr.MASH, CONTAINMENT: cr.CONTAINMENT, MAX_CONTAINMENT: cr.MAX_CONTAINMENT}[bit])


def columns(orc, mask, dot, nr, nq, k):
    """the (n, popcount(mask)) array hg_ani_pairs writes for n pairs given as arrays of (dot, nr, nq)"""
    dot, nr, nq = (np.ascontiguousarray(v, np.int32).ravel() for v in (dot, nr, nq))
    cols = [column(orc, b, dot, nr, nq, k) for b in BITS if mask & b]
    return np.stack(cols, 1) if cols else np.zeros((dot.size, 0), np.float32)


def place(mask, bit):
    """index of column `bit` among a pair's values under `mask`"""
    return bin(mask & (bit - 1)).count("1")


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and bool((a.view(np.uint32) == b.view(np.uint32)).all())


def fmt3(a):
    """the CLI's "{:.3}" of a float32 ANI (hg_cli.cpp: put_ani)"""
    v = int(np.rint(float(min(max(float(a), 0.0), 100.0)) * 1000.0))
    return "%d.%03d" % (v // 1000, v % 1000)
