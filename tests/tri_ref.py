"""The reference of libhypergen_tri.so (include/hypergen_tri.h) in numpy: the integer a pair prints, the 8-byte field, the field
text of a block of rows in both layouts, the closed-form sizes and offsets in Python's unbounded integers, and the matrix file
`hyper-gen triangle` writes -- from a matrix of integers, or from the TSV of the same file's `dist -a 0`."""
import numpy as np

LOWER, FULL = 0, 1
FIELD = 8
MILLI_MAX = 100_000


class Invalid(Exception):
    pass


def milli(ani):
    """hg_avg_milli: NaN and negative values 0, values above 100 100 000, else the product with 1000 -- exact in a double --
    rounded to the nearest integer, ties to even"""
    a = np.asarray(ani, np.float32).astype(np.float64)
    a = np.where(a >= 0.0, a, 0.0)  # NaN too
    a = np.minimum(a, 100.0)
    return np.rint(a * 1000.0).astype(np.int64)


def field(m, last=False):
    """the 8 bytes of one field: "%3d.%03d" and the separator"""
    if not 0 <= m <= MILLI_MAX:
        raise Invalid(m)
    return b"%3d.%03d%c" % (m // 1000, m % 1000, b"\n" if last else b"\t")


def tri(i):
    """the fields in front of row i under LOWER"""
    return i * (i - 1) // 2 if i else 0


def text_bytes(layout, row0, rows, cols):
    if layout == LOWER:
        return FIELD * (tri(row0 + rows) - tri(row0))
    if layout == FULL:
        return FIELD * rows * cols
    raise Invalid(layout)


def field_offset(layout, row0, i, j, cols):
    if layout == LOWER:
        return FIELD * (tri(i) - tri(row0) + j)
    if layout == FULL:
        return FIELD * ((i - row0) * cols + j)
    raise Invalid(layout)


def fields_of_milli(m, last_col=None):
    """(rows, cols) integers as a (rows, cols, 8) uint8 array of fields, '\\t' everywhere but in column last_col[r] of row r"""
    m = np.asarray(m, np.int64)
    rows, cols = m.shape
    out = np.empty((rows, cols, FIELD), np.uint8)
    ip, fp = m // 1000, m % 1000
    digit = lambda v: (v + ord("0")).astype(np.uint8)
    out[..., 0] = np.where(ip >= 100, ord("1"), ord(" "))
    out[..., 1] = np.where(ip >= 10, digit(ip // 10 % 10), ord(" "))
    out[..., 2] = digit(ip % 10)
    out[..., 3] = ord(".")
    out[..., 4], out[..., 5], out[..., 6] = digit(fp // 100), digit(fp // 10 % 10), digit(fp % 10)
    out[..., 7] = ord("\t")
    if last_col is not None:
        for r in range(rows):
            if 0 <= last_col[r] < cols:
                out[r, last_col[r], 7] = ord("\n")
    return out


def block_text(ani, layout, row0=0):
    """the field text of a block of floats whose columns start at global column 0 and whose row r is global row row0 + r (bytes)"""
    ani = np.asarray(ani, np.float32)
    rows, cols = ani.shape
    if layout == FULL:
        return fields_of_milli(milli(ani), [cols - 1] * rows).tobytes()
    if layout != LOWER:
        raise Invalid(layout)
    if rows and cols < row0 + rows - 1:
        raise Invalid("LOWER needs cols >= row0 + rows - 1")
    f = fields_of_milli(milli(ani), [row0 + r - 1 for r in range(rows)])
    return b"".join(f[r, : row0 + r].tobytes() for r in range(rows))


def file_text(names, m, layout):
    """the file of `hyper-gen triangle`: names as bytes, m an (n, n) array of integers of which LOWER reads j < i"""
    n = len(names)
    out = [b"%d\n" % n]
    for i, name in enumerate(names):
        cols = i if layout == LOWER else n
        out.append(name + (b"\t" if cols else b"\n"))
        out.append(b"".join(field(int(m[i][j]), j == cols - 1) for j in range(cols)))
    return b"".join(out)


def file_from_tsv(names, tsv, layout):
    """the same from the TSV `dist -a 0` writes for the file against itself: "a<TAB>b<TAB>ani" per pair.  Under a symmetric metric
    (LOWER) dist writes every unordered pair once, under containment (FULL) every ordered pair i != j as reference i, query j
    and the diagonal reads 100.000.  The names must be distinct."""
    at = {name: k for k, name in enumerate(names)}
    if len(at) != len(names):
        raise Invalid("names repeat")
    n = len(names)
    m = np.full((n, n), -1, np.int64)
    for line in tsv.split(b"\n"):
        if not line:
            continue
        a, b, v = line.rsplit(b"\t", 2)
        ip, fp = v.split(b".")
        if len(fp) != 3:
            raise Invalid(v)
        val = int(ip) * 1000 + int(fp)
        i, j = at[a], at[b]
        if m[i, j] != -1:
            raise Invalid("pair twice: %r" % line)
        m[i, j] = val
        if layout == LOWER:
            if m[j, i] != -1:
                raise Invalid("pair twice: %r" % line)
            m[j, i] = val
    if layout == FULL:
        np.fill_diagonal(m, MILLI_MAX)
    need = np.tril(np.ones((n, n), bool), -1) if layout == LOWER else np.ones((n, n), bool)
    if (m[need] < 0).any():
        raise Invalid("the TSV lacks pairs")
    return file_text(names, m, layout)
