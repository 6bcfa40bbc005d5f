"""The numpy reading of include/hypergen_frag.h, for the tests of libhypergen_frag.so and of the command line built on it: the
window plan, the integer m of an ANI, the bests with their tie rule, the fold per pair of genomes, the ANI integer, the
grouping of record names into genomes and the two text files `dist --fragments` writes.  Nothing here calls the library."""
import re

import numpy as np

PAIR_DTYPE = np.dtype([("sum", np.uint64), ("matched", np.uint32), ("total", np.uint32)])
BEST_DTYPE = np.dtype([("m", np.uint32), ("row", np.uint32)])
NONE = 0xFFFFFFFF


class Invalid(ValueError):
    """what the library answers with HG_ERR_INVALID"""


def plan(length, window, step):
    """[(start, len)] of the windows of a sequence of `length` bases"""
    if window % 4 or step % 4 or step < 4 or step > window:
        raise Invalid("window and step")
    if length <= window:
        return [(0, length)]
    out = []
    start = 0
    while True:  # a window starts every `step` bases until one reaches the end
        out.append((start, min(window, length - start)))
        if start + window >= length:
            break
        start += step
    if len(out) > 1 and 2 * out[-1][1] < window:
        out.pop()
    return out


def milli(ani):
    """m of an array of float32 ANIs: NaN and negative 0, above 100 100 000, else the product with 1000 rounded half to even"""
    a = np.asarray(ani, np.float32).astype(np.float64)
    a = np.where(np.isnan(a) | (a < 0), 0.0, a)
    a = np.minimum(a, 100.0)
    return np.rint(a * 1000.0).astype(np.uint32)


def threshold(frag_th):
    return int(milli(np.float32(frag_th)))


def check_offsets(first, end):
    first = np.asarray(first, np.int64)
    if first.size == 0:
        if end:
            raise Invalid("no genome")
        return first
    if first[0] != 0 or first[-1] != end or (np.diff(first) < 0).any():
        raise Invalid("offsets")
    return first


def bests(ani, ref_first):
    """best(g, q) of an R x Q matrix: BEST_DTYPE [n_ref, Q]; the smallest row wins a tie, a genome without rows is {0, NONE}"""
    ani = np.asarray(ani, np.float32)
    R, Q = ani.shape
    rf = check_offsets(ref_first, R)
    n_ref = max(rf.size - 1, 0)
    out = np.zeros((n_ref, Q), BEST_DTYPE)
    out["row"] = NONE
    m = milli(ani)
    for g in range(n_ref):
        lo, hi = int(rf[g]), int(rf[g + 1])
        if hi > lo and Q:
            seg = m[lo:hi]
            arg = seg.argmax(axis=0)  # (the first maximum: the smallest row)
            out["m"][g] = seg[arg, np.arange(Q)]
            out["row"][g] = lo + arg
    return out


def fold(best, qry_first, frag_th, R=None):
    """pair(g, h) from the bests: PAIR_DTYPE [n_ref, n_qry].  R == 0 (or no column): the records of an empty comparison."""
    n_ref, Q = best.shape
    qf = check_offsets(qry_first, Q)
    n_qry = max(qf.size - 1, 0)
    out = np.zeros((n_ref, n_qry), PAIR_DTYPE)
    m_th = threshold(frag_th)
    for h in range(n_qry):
        lo, hi = int(qf[h]), int(qf[h + 1])
        out["total"][:, h] = hi - lo
        if R == 0 or Q == 0:
            continue
        seg = best["m"][:, lo:hi].astype(np.uint64)
        ok = seg >= m_th
        out["matched"][:, h] = ok.sum(axis=1)
        out["sum"][:, h] = (seg * ok).sum(axis=1)
    return out


def reduce(ani, ref_first, qry_first, frag_th):
    """(pair records, best records) of hg_frag_ani_matrix_dev on this matrix"""
    ani = np.asarray(ani, np.float32)
    b = bests(ani, ref_first)
    return fold(b, qry_first, frag_th, R=ani.shape[0]), b


def ani_milli(sum_, matched):
    """the genome ANI in thousandths: the mean of the matched bests, rounded half up, in integer arithmetic"""
    return (2 * int(sum_) + int(matched)) // (2 * int(matched))


def milli_str(v):
    return "%d.%03d" % (v // 1000, v % 1000)


_SUFFIX = re.compile(r"\A(.*):[0-9]+-[0-9]+\Z", re.S)


def genome_of(name):
    m = _SUFFIX.match(name)
    return m.group(1) if m and m.group(1) != "" else name


def genomes(names):
    """(first, genome names): consecutive records of one genome; a genome that reappears behind another raises Invalid"""
    first, out = [], []
    for i, name in enumerate(names):
        g = genome_of(name)
        if out and out[-1] == g:
            continue
        if g in out:
            raise Invalid("genome %r reappears at record %r" % (g, name))
        first.append(i), out.append(g)
    first.append(len(names))
    return first, out


def tsv(pair, ref_names, qry_names, ani_th, min_fragments=1):
    """the lines of -o: by query, then reference: ref, qry, ANI, matched, total"""
    a = threshold(ani_th)
    lines = []
    for h, qn in enumerate(qry_names):
        for g, rn in enumerate(ref_names):
            p = pair[g, h]
            if p["matched"] == 0 or p["matched"] < min_fragments:
                continue
            v = ani_milli(p["sum"], p["matched"])
            if v >= a:
                lines.append("%s\t%s\t%s\t%d\t%d\n" % (rn, qn, milli_str(v), p["matched"], p["total"]))
    return "".join(lines)


def hits(best, ref_records, qry_records, frag_th):
    """the lines of --fragment_hits: by query fragment, then reference genome: fragment, its best window, ANI"""
    m_th = threshold(frag_th)
    lines = []
    for q, qn in enumerate(qry_records):
        for g in range(best.shape[0]):
            b = best[g, q]
            if b["row"] != NONE and b["m"] >= m_th:
                lines.append("%s\t%s\t%s\n" % (qn, ref_records[int(b["row"])], milli_str(int(b["m"]))))
    return "".join(lines)
