"""Crafted inputs for the FracMinHash sampling edge tests (test_gpu_sampling_edges.py on the device, test_sampling_construction.py
on the host).  Everything is generated from fixed seeds; the only hash function used is the oracle's.

The decision under test is `keep h  <=>  h < threshold` (threshold = (2^64 - 1) // scaled) and the route a kept hash takes in the
k-mer kernels (hyper-gen_amd/csrc/hg_kmer_hits.h): the work item's LDS list of STAGE entries, one global atomic per wave once
it overflows (append_hit), quarter-full flushes between tiles when dense_sampling(threshold), the per-genome hit region of
2 * expect + 1 024 slots (hg_sketch_plan.hip) and the re-run of a genome that overflows it.

Dense genomes are built from DISTINCT sampled k-mers (hash below the threshold of scaled = 1 500, so below every threshold used
here), cut out of seeded random ACGT: a k-mer keeps its hash wherever it is placed.  "dirty" puts one N behind every k-mer (the
sampled set of the stretch is exactly the chosen hashes), "clean" concatenates them (the windows across the joins add their own).
"""
import numpy as np

MAX = 2**64 - 1
DENSE_EDGE = MAX // 850  # dense_sampling(threshold) <=> threshold > DENSE_EDGE: scaled <= 849
STAGE = 256              # entries of a work item's LDS hit list at every threshold used for the dense genomes
SPARSE = 1500
B_SCALED = (1500, 851, 850, 849)   # both sides of the dense_sampling switch
B_KS = (21, 28, 33, 40, 64, 100)   # kmer_sample_shared (two code windows), kmer_sample_long<K>, run-time k
ACGT = np.frombuffer(b"ACGT", np.uint8)
N = ord("N")


def thr(scaled):
    return MAX // scaled


def item_starts(k):
    """k-mer starts per work item (hg_kmer_item_starts; pinned against hg_sketch_plan_describe by the CPU module)"""
    return 27432 if k <= 21 else 27324 if k <= 32 else 12288


def tile_starts(k):
    return item_starts(k) // 9 if k <= 32 else 1536


def window_hashes(orc, seq, k, canonical=True, seed=123):
    """(start, hash) of every window of k bases without a non-ACGT byte, in window order"""
    s = np.asarray(seq, np.uint8)
    h = orc.kmer_hash_sample(s, k, threshold=MAX, seed=seed, canonical=canonical, unique=False)
    nw = max(0, s.size - k + 1)
    bad = np.concatenate([[0], np.cumsum(~np.isin(s, ACGT))])
    pos = np.flatnonzero(bad[k:k + nw] == bad[:nw])
    assert pos.size == h.size, (pos.size, h.size)  # (no window hashes to 2^64 - 1: the oracle could not keep it)
    return pos, h


def dense_count(k):
    """distinct sampled k-mers in one dense stretch: two work items' worth of dirty k-mers, and enough to overflow the genome's
    hit region (2 * L / 849 + 1 024 slots for a genome of L ~ count * (k + 1) bases, plus the random flanks)"""
    return max(-(-2 * item_starts(k) // (k + 1)), int(1300 / (1 - 2 * (k + 1) / 849.0)) + 1)


_POOLS = {}


def sampled_pool(orc, k, canonical):
    """(kmers[n, k], hashes[n]): n = dense_count(k) distinct k-mers sampled at scaled = 1 500"""
    key = (k, canonical)
    if key not in _POOLS:
        n = dense_count(k)
        rng = np.random.default_rng(9100 + 2 * k + int(canonical))
        seq = rng.choice(ACGT, int(n * SPARSE * 1.3) + 20_000)
        h = orc.kmer_hash_sample(seq, k, threshold=MAX, canonical=canonical, unique=False)  # pure ACGT: hash i = window i
        idx = np.flatnonzero(h < np.uint64(thr(SPARSE)))
        _, first = np.unique(h[idx], return_index=True)
        idx = np.sort(idx[first])
        assert idx.size >= n, (k, idx.size, n)
        idx = idx[:n]
        _POOLS[key] = (seq[idx[:, None] + np.arange(k)], h[idx])
    return _POOLS[key]


def stretch(kmers, clean):
    if clean:
        return kmers.reshape(-1)
    return np.concatenate([kmers, np.full((len(kmers), 1), N, np.uint8)], axis=1).reshape(-1)


def dense_batch(orc, k, canonical, clean):
    """A mixed batch: (genomes, roles, chosen) with
      "head"    the dense stretch at the start of the genome,
      "across"  the stretch starting a quarter into the first work item, across tile and work-item boundaries,
      "tail"    the stretch as the genome's last k-mers,
      "plain"   ordinary random genomes (a 90 kbp one, then small ones of 1.5 - 3 kbp),
      "small"   one genome of ~2.5 kbp made of dirty sampled k-mers in the middle of the small ones (k <= 32: one workgroup
                takes all of them; its hits must not land in its neighbours' lists, nor theirs in its list).
    chosen[i]: the pool hashes placed in genome i (None for the plain ones)."""
    kmers, hashes = sampled_pool(orc, k, canonical)
    n = len(kmers)
    rng = np.random.default_rng(9300 + 4 * k + 2 * int(canonical) + int(clean))
    body = lambda sh: stretch(np.roll(kmers, sh, axis=0), clean)  # noqa: E731  (another k-mer order per genome)
    chosen_all = lambda sh: np.roll(hashes, sh)  # noqa: E731
    head = np.concatenate([body(0), rng.choice(ACGT, 5_000)])
    pre = item_starts(k) // 4 + 17
    across = np.concatenate([rng.choice(ACGT, pre), body(n // 3), rng.choice(ACGT, 4_000)])
    tail = np.concatenate([rng.choice(ACGT, 7_000), body(2 * n // 3)])
    if not clean:
        tail = tail[:-1]  # (ends with the last k-mer, not with its N)
    n_small = 2_500 // (k + 1)
    small = stretch(kmers[:n_small], False)[:-1]
    genomes = [head, across, tail, rng.choice(ACGT, 90_000)]
    roles = ["head", "across", "tail", "plain"]
    chosen = [chosen_all(0), chosen_all(n // 3), chosen_all(2 * n // 3), None]
    for i in range(13):
        if i == 6:
            genomes.append(small), roles.append("small"), chosen.append(hashes[:n_small])
        else:
            genomes.append(rng.choice(ACGT, int(rng.integers(1_500, 3_000)))), roles.append("plain"), chosen.append(None)
    return genomes, roles, chosen


def offsets_for(lens):
    return np.concatenate([[0], np.cumsum((np.asarray(lens, np.uint64) + 15) // 16 * 16)[:-1]]).astype(np.uint64)
