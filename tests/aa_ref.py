"""Reference for the amino-acid sketch (include/hypergen_aa.h), built from the oracle's primitives alone: windows in Python,
orc_t1ha2_atonce on the upper-cased bytes, the threshold, sorted(set(...)), then oracle.encode_hv / hv_norm2 / ani_from_dot.
Nothing here comes from the code under test."""
import ctypes as C

import numpy as np

from oracle import oracle as orc

RESIDUES = frozenset(b"ACDEFGHIKLMNPQRSTVWY" + b"acdefghiklmnpqrstvwy")
U64_MAX = 2**64 - 1


def _arr(seq):
    return np.frombuffer(bytes(seq), np.uint8) if not isinstance(seq, np.ndarray) else np.ascontiguousarray(seq, np.uint8)


def window_hashes(seq, k, seed=123):
    """[(start, hash)] of every window of k residues, in order of start"""
    a = _arr(seq)
    ok = np.fromiter((int(b) in RESIDUES for b in a), bool, a.size)
    up = np.where(ok, a & 0xDF, a).astype(np.uint8)
    if a.size < k:
        return []
    bad = np.concatenate(([0], np.cumsum(~ok)))
    starts = np.nonzero(bad[k:] == bad[:-k])[0]  # no non-residue in [i, i + k)
    fn, base = orc.lib().orc_t1ha2_atonce, up.ctypes.data
    u8p, s = C.POINTER(C.c_uint8), C.c_uint64(seed)
    return [(int(i), int(fn(C.cast(base + int(i), u8p), k, s))) for i in starts]


def hash_sample(seq, k, scaled=1500, seed=123, threshold=None):
    """the distinct kept hashes, ascending (uint64)"""
    thr = U64_MAX // scaled if threshold is None else threshold
    return np.array(sorted({h for _, h in window_hashes(seq, k, seed) if h < thr}), np.uint64)


def sketch(seq, k, scaled=1500, seed=123, hv_d=4096, layout=orc.LAYOUT_AVX2):
    """(hv, norm2, nhash)"""
    hs = hash_sample(seq, k, scaled, seed)
    hv = orc.encode_hv(hs, hv_d, layout)
    return hv, orc.hv_norm2(hv), int(hs.size)


def aai(hv_a, hv_b, k):
    dot = int(np.dot(hv_a.astype(np.int64), hv_b.astype(np.int64)))
    return orc.ani_from_dot(dot, orc.hv_norm2(hv_a), orc.hv_norm2(hv_b), k)


def parse_fasta(data):
    """hg_aa_read_fasta's layout from the bytes of a plain FASTA file: one '*' per record start, line ends / blanks / tabs / CRs dropped"""
    out = bytearray()
    for line in data.split(b"\n"):
        if line.startswith(b">"):
            out += b"*"
        else:
            out += bytes(b for b in line if b not in b"\r \t")
    return bytes(out)
