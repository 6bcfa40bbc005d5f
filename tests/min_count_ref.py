"""The reference for hg_sketch_params.min_count: with raw the multiset of sampled hashes of a sequence (one per sampled k-mer
position, orc.kmer_hash_sample(..., unique=False)) and m = max(1, min_count), kept = the hashes that occur at least m times,
ascending; the sketch is the oracle's encoding of kept.  The only hash function here is the oracle's."""
import numpy as np


def kept(raw, m):
    vals, counts = np.unique(np.asarray(raw, np.uint64), return_counts=True)
    return vals[counts >= max(1, int(m))]


def sketch(orc, seq, m, ksize=21, scaled=1500, seed=123, canonical=True, norm=0, hv_d=4096, layout=1):
    """(hv, norm2, nhash, kept) of one sequence under min_count = m"""
    raw = orc.kmer_hash_sample(seq, ksize, scaled, seed=seed, canonical=canonical, norm=norm, unique=False)
    k = kept(raw, m)
    hv = orc.encode_hv(k, hv_d, layout)
    return hv, orc.hv_norm2(hv), int(k.size), k


def read_set(seed=7, L=300_000, cov=30, rl=150, err=0.01):
    """The seeded read set of the README's min_count table: (reads, genome) as ASCII, every read (and the genome) behind an N.
    30x coverage of 150-base reads with 1 % substitutions, half of them reverse-complemented."""
    rng = np.random.default_rng(seed)
    g = rng.integers(0, 4, L).astype(np.uint8)
    A = np.frombuffer(b"ACGT", np.uint8)
    comp = np.array([3, 2, 1, 0], np.uint8)
    n = L * cov // rl
    starts = rng.integers(0, L - rl, n)
    buf = np.empty(n * (rl + 1), np.uint8)
    for i, s in enumerate(starts):
        r = g[s:s + rl].copy()
        e = rng.random(rl) < err
        r[e] = (r[e] + rng.integers(1, 4, e.sum())) % 4
        if rng.random() < 0.5:
            r = comp[r[::-1]]
        buf[i * (rl + 1)] = ord("N")
        buf[i * (rl + 1) + 1:(i + 1) * (rl + 1)] = A[r]
    genome = np.concatenate([[ord("N")], A[g]]).astype(np.uint8)
    return buf, genome
