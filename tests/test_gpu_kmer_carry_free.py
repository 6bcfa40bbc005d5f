"""The 128-bit products with P1 and P3 in the k-mer kernels have no carry op (hg_kmer_t1ha2.h: mul128_cross_fits).  No
operand can set the carry that was removed -- that is arithmetic, checked by the file's static_asserts and by
test_mul128_carry_free.py -- so what is tested here is the text itself: the asm statements of k = 17..32 (HG_KS_MUL128_NC in
the P1 stage, in the P3 stage of k >= 25 and in the general first mixup of k <= 24; their register binding, and VCC, which the
neighbouring P2 stage and final64 still use), the C++ path of k <= 16, and the constant-k tails of kmer_sample_long.

Exact equality of whole hash sets with the CPU oracle at threshold 2^64 - 1, which keeps every k-mer.  k covers the C++ path
(12, 16), both asm texts with every width class of the last word (17, 21, 24 / 25, 29, 32) and tails of one, two and no stages
behind the long kernel's rounds (33, 48, 64).  Seeds lie on both sides of 2^28 (bounded and general first mixup), and the
large ones make s + w0 wrap 64 bits.  Inputs are two tiles of one work item, the second an edge tile: random ACGT, all T, all
A, and a sequence with lower case, N and U (a dirty tile: the second copy of the k-mer loop)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ACGT = np.frombuffer(b"ACGT", np.uint8)
N_BASES = 7000
ALL = 2**64 - 1
SEEDS = (0, 123, 2**28 - 1, 2**28, 2**63 + 11, 2**64 - 1)
KS = (12, 16, 17, 21, 24, 25, 29, 32, 33, 48, 64)


@pytest.fixture(scope="module")
def hg():
    import hypergen_amd
    return hypergen_amd


@pytest.fixture(scope="module")
def ctxs(hg):
    """one ctx per input form of hg_kmer_hash_sample: ASCII and hg_pack2 blobs"""
    out = {}
    for form in ("ascii", "packed"):
        c = hg.Context(0)
        c.set_stream(torch.cuda.current_stream().cuda_stream)
        c.set_debug("hostfed", form)
        out[form] = c
    yield out
    for c in out.values():
        c.close()


@pytest.fixture(scope="module")
def inputs():
    rng = np.random.default_rng(1212)
    rnd = rng.choice(ACGT, N_BASES).astype(np.uint8)
    mixed = rng.choice(ACGT, N_BASES).astype(np.uint8)
    mixed[100:160] |= 0x20                      # a lower-case run: still bases
    mixed[3040:3060] |= 0x20                    # ... across the tile boundary
    for at in (7, 500, 501, 3050, 6990):
        mixed[at] = ord("N")
    mixed[1234] = ord("U")
    mixed[4321] = ord("u")
    return {"random": rnd, "all_T": np.full(N_BASES, ord("T"), np.uint8), "all_A": np.full(N_BASES, ord("A"), np.uint8),
            "mixed": mixed}


def kernel_name(k, canonical, packed):
    if k > 32:
        return "kmer_sample_long<%d, %s>" % (k, "true" if packed else "false")
    return "kmer_sample_shared<%d, %s, %s>" % (k, "true" if canonical else "false", "true" if packed else "false")


@pytest.mark.parametrize("canonical", [True, False], ids=["canon", "fwd"])
@pytest.mark.parametrize("k", KS)
def test_whole_hash_set(ctxs, orc, inputs, k, canonical):
    for name, s in inputs.items():
        for norm in ((0, 1) if name == "mixed" else (0,)):  # u/U: a non-base, or a T under HG_NORM_U2T
            for seed in SEEDS:
                want = orc.kmer_hash_sample(s, k, 1, seed, canonical, norm, threshold=ALL)
                assert want.size > 0
                for form, c in ctxs.items():
                    got = c.kmer_hash_sample(s, k, 1, seed, canonical, norm, threshold=ALL, cap=N_BASES + 64)
                    assert c.last_kernel("kmer") == kernel_name(k, canonical, form == "packed")
                    assert got.size == want.size and (got == want).all(), (name, norm, hex(seed), form, got.size, want.size)
