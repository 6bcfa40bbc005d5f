"""The k = 17..32 k-mer kernels test the threshold in two steps: a lane is a candidate when hi32(h) <= hi32(threshold) (one
32-bit compare inside the hash's asm), and the wave-uniform hit path keeps it when h < threshold.  Here the thresholds share
their high dword with sampled hashes and put the low dword on either side of the hash's, and the k-mers carrying those hashes
are planted many times on both strands, so that whole waves are candidates that the exact test must drop or keep.

Also the strand choice for odd k, which compares the top 16 bases of the two strands only: sequences rich in reverse-complement
palindromes (whose strands agree as far as the middle base) must give the oracle's canonical hashes.
"""
import numpy as np
import pytest

from sampling_craft import MAX, window_hashes

pytestmark = pytest.mark.gpu

KS = (17, 19, 21, 23, 24, 25, 31, 32)
LO = 0xFFFFFFFF
ACGT = np.frombuffer(b"ACGT", np.uint8)
COMP = np.zeros(256, np.uint8)
COMP[list(b"ACGT")] = list(b"TGCA")


@pytest.fixture(scope="module")
def hg():
    import hypergen_amd
    return hypergen_amd


@pytest.fixture(scope="module", params=["ascii", "packed"])
def ctx(hg, request):
    c = hg.Context(0)
    c.set_debug("kmer_input", "packed" if request.param == "packed" else "")
    yield c
    c.close()


def revcomp(s):
    return COMP[s[::-1]]


def planted(orc, k, canonical, seed):
    """random ACGT with three k-mers of small hash planted 40 times each (forward and, for canonical, reverse complement)"""
    rng = np.random.default_rng(7100 + 2 * k + int(canonical))
    src = rng.choice(ACGT, 200_000)
    pos, h = window_hashes(orc, src, k, canonical, seed)
    picks = pos[np.argsort(h)[[3, 11, 29]]]
    s = rng.choice(ACGT, 30_000 + 7 * k)
    for i, p in enumerate(np.repeat(picks, 40)):
        km = src[p:p + k]
        at = int(rng.integers(0, s.size - k))
        s[at:at + k] = revcomp(km) if canonical and i % 2 else km
    return s


def check(ctx, orc, s, k, canonical, seed, thresholds):
    u = np.unique(window_hashes(orc, s, k, canonical, seed)[1])
    for t in thresholds:
        want = u[:int(np.searchsorted(u, np.uint64(t), "left"))]
        got = ctx.kmer_hash_sample(s, k, seed=seed, canonical=canonical, threshold=t, cap=u.size + 64)
        assert got.size == want.size and (got == want).all(), (k, canonical, seed, hex(t), got.size, want.size)
    return u


@pytest.mark.parametrize("seed", [123, 2**32 - 1])
@pytest.mark.parametrize("canonical", [True, False], ids=["canon", "fwd"])
@pytest.mark.parametrize("k", KS)
def test_threshold_high_dword_equal(ctx, orc, k, canonical, seed):
    s = planted(orc, k, canonical, seed)
    u = np.unique(window_hashes(orc, s, k, canonical, seed)[1])
    ts = set()
    for h in (int(x) for x in u[[3, 11, 29, u.size // 2]]):
        hi, lo = h & ~LO, h & LO
        # same high dword; the hash's low dword below, equal to and above the threshold's
        for tl in (0, lo - 1, lo, lo + 1, LO, lo // 2, (lo + LO + 1) // 2):
            if 0 <= tl <= LO:
                ts.add(hi | tl)
    check(ctx, orc, s, k, canonical, seed, sorted(ts))


@pytest.mark.parametrize("k", [k for k in KS if k % 2 == 1])
def test_odd_k_strand_palindromes(ctx, orc, k):
    """k-mers whose two strands share their first (k - 1) / 2 bases, and palindromic stretches whose windows do"""
    rng = np.random.default_rng(7300 + k)
    parts = []
    for _ in range(600):
        half = rng.choice(ACGT, (k - 1) // 2)
        mid = rng.choice(ACGT, 1)
        parts += [half, mid, revcomp(half), rng.choice(ACGT, int(rng.integers(0, 9)))]
    for _ in range(200):
        half = rng.choice(ACGT, int(rng.integers(k // 2, 2 * k)))
        parts += [half, revcomp(half), rng.choice(ACGT, int(rng.integers(0, 5)))]
    s = np.concatenate(parts)
    u = np.unique(window_hashes(orc, s, k, True, 123)[1])
    check(ctx, orc, s, k, True, 123, [MAX, int(u[u.size // 3]), int(u[u.size // 2]) & ~LO])
