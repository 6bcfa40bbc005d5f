"""The numpy reading of include/hypergen_hist.h, for the tests of libhypergen_hist.so and of `hyper-gen dist --histogram`: the bins
of a width, the selection of pairs by their global indices, the counts of a matrix, the counts of the third field of a dist
TSV and the file the command line writes.  The integer m of an ANI is frag_ref.milli, the restatement of hg_avg_milli the
fragment tests use.  Nothing here calls the library."""
import numpy as np

from frag_ref import Invalid, milli, milli_str

ALL, UPPER, OFFDIAG = 0, 1, 2
MILLI_MAX = 100_000


def bins(bin_milli):
    """n_bins of a width in thousandths, 0 for a width outside 1..100 000"""
    return MILLI_MAX // bin_milli + 1 if 1 <= bin_milli <= MILLI_MAX else 0


def selected(rows, cols, row0, col0, pairs):
    """bool [rows, cols]: which entries of a block at (row0, col0) count"""
    i = row0 + np.arange(rows, dtype=np.int64)[:, None]
    j = col0 + np.arange(cols, dtype=np.int64)[None, :]
    if pairs == ALL:
        return np.ones((rows, cols), bool)
    if pairs == UPPER:
        return i < j
    if pairs == OFFDIAG:
        return i != j
    raise Invalid("pairs")


def counts_of_milli(m, bin_milli):
    """uint64 [n_bins] of integers 0..100 000"""
    n = bins(bin_milli)
    if not n:
        raise Invalid("bin_milli")
    m = np.asarray(m, np.int64).reshape(-1)
    assert m.size == 0 or (0 <= m.min() and m.max() <= MILLI_MAX)
    return np.bincount(m // bin_milli, minlength=n).astype(np.uint64)


def counts(ani, bin_milli, pairs=ALL, row0=0, col0=0):
    """what hg_hist_add_matrix_dev adds for this block (a 2-d array; a pitch is the caller's slicing)"""
    ani = np.asarray(ani, np.float32)
    return counts_of_milli(milli(ani)[selected(ani.shape[0], ani.shape[1], row0, col0, pairs)], bin_milli)


def parse_bin(text):
    """--histogram_bin as the command line reads it: a decimal string into thousandths, exactly"""
    ip, _, fp = text.partition(".")
    if not (ip + fp) or not (ip + fp).isdigit() or not (ip + fp).isascii() or len(fp) > 3 or len(ip) > 6:
        raise Invalid(text)
    v = int(ip or "0") * 1000 + int((fp + "000")[:3])
    if not bins(v):
        raise Invalid(text)
    return v


def tsv_milli(tsv):
    """the third field of every line of a dist TSV, in thousandths (the fields print three decimals)"""
    out = []
    for line in tsv.splitlines():
        ip, fp = line.split("\t")[2].split(".")
        assert len(fp) == 3
        out.append(int(ip) * 1000 + int(fp))
    return np.array(out, np.int64)


def file_text(c, bin_milli):
    """the lines of --histogram: lo, hi, count, count of this and all higher bins"""
    c = [int(x) for x in c]
    assert len(c) == bins(bin_milli)
    above = np.cumsum(c[::-1], dtype=object)[::-1] if c else []
    return "".join("%s\t%s\t%d\t%d\n" % (milli_str(b * bin_milli), milli_str(min((b + 1) * bin_milli - 1, MILLI_MAX)), c[b], above[b])
                   for b in range(len(c)))
