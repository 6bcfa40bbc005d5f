"""Reference for the six-frame translated sketch (include/hypergen_tx.h), built from the oracle's primitives alone: the codon
string of NCBI table 1, frames by Python slicing and a reverse complement, then aa_ref.window_hashes on each of the six frame
strings and the union.  Nothing here comes from the code under test."""
import numpy as np

import aa_ref
from oracle import oracle as orc

CODONS = "FFLLSSSSYY**CC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG"  # index 16 b1 + 4 b2 + b3, bases ordered T C A G
RANK = {ord(c): i for i, c in enumerate("TCAG")}
RANK.update({ord(c): i for i, c in enumerate("tcag")})
COMP = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")  # every other byte stays what it is: a non-base at its mirrored place
U64_MAX = aa_ref.U64_MAX


def _bytes(seq):
    return seq.tobytes() if isinstance(seq, np.ndarray) else bytes(seq)


def revcomp(seq):
    return _bytes(seq).translate(COMP)[::-1]


def translate(s):
    """the residues of the codons s[0:3], s[3:6], ...: '*' a stop, 'X' a codon with a non-base in it"""
    out = bytearray()
    for j in range(0, len(s) - 2, 3):
        r = [RANK.get(b) for b in s[j:j + 3]]
        out.append(ord("X") if None in r else ord(CODONS[16 * r[0] + 4 * r[1] + r[2]]))
    return bytes(out)


def frames(seq):
    """the six frame strings: 0..2 forward, 3..5 those of the reverse complement"""
    s = _bytes(seq)
    rc = revcomp(s)
    return [translate(s[f:]) for f in range(3)] + [translate(rc[f:]) for f in range(3)]


def frame_windows(seq, k, seed=123):
    """per frame: [(residue start, hash)] of every window of k residues ('*' and 'X' are no residues for aa_ref)"""
    return [aa_ref.window_hashes(fr, k, seed) for fr in frames(seq)]


def hash_sample(seq, k, scaled=1500, seed=123, threshold=None):
    """the distinct kept hashes over all six frames, ascending (uint64)"""
    thr = U64_MAX // scaled if threshold is None else threshold
    return np.array(sorted({h for fw in frame_windows(seq, k, seed) for _, h in fw if h < thr}), np.uint64)


def prefix_sets(seq, k, lengths, scaled=1500, seed=123):
    """hash_sample of seq[:L] for every L of lengths, from one pass over seq: a forward window of frame f at residue j
    spans the bases [f + 3j, f + 3j + 3k); a window of frame 3 + f of seq[:L] is the reverse complement of the bases
    [p, p + 3k) with p + 3k <= L, whatever L is -- so both strands are taken per nucleotide start p of the whole seq."""
    s = _bytes(seq)
    thr = U64_MAX // scaled
    by_start = []  # (p, hash) of every kept k-mer, both strands
    for f in range(3):
        by_start += [(f + 3 * j, h) for j, h in aa_ref.window_hashes(translate(s[f:]), k, seed) if h < thr]
    n = len(s)
    rc = revcomp(s)
    for f in range(3):  # residue j of frame f of rc covers rc[f + 3j, f + 3j + 3k) = the bases [n - f - 3j - 3k, n - f - 3j) of s
        by_start += [(n - f - 3 * j - 3 * k, h) for j, h in aa_ref.window_hashes(translate(rc[f:]), k, seed) if h < thr]
    p = np.array([x for x, _ in by_start], np.int64)
    h = np.array([x for _, x in by_start], np.uint64)
    return [np.unique(h[p + 3 * k <= L]) for L in lengths]


def sketch(seq, k, scaled=1500, seed=123, hv_d=4096, layout=orc.LAYOUT_AVX2):
    """(hv, norm2, nhash)"""
    hs = hash_sample(seq, k, scaled, seed)
    hv = orc.encode_hv(hs, hv_d, layout)
    return hv, orc.hv_norm2(hv), int(hs.size)
