"""The 128-bit products of t1ha2's mixups with P1 and P3 run without a carry op (hg_kmer_t1ha2.h: mul128_cross_fits and
that path of mul128_lo_hiadd; hg_kmer_asm.h: HG_KS_MUL128_NC).  The schoolbook product sums x0 p1 + x1 p0 + hi32(x0 p0) in 64 bits;
for a prime with p0 + p1 < 2^32 that sum cannot reach 2^64, whatever x is, so its carry-out is never set.

Here, in Python integers: the predicate's arithmetic for P0..P6, and the six-instruction sequence restated register by
register -- every step masked to the 32 or 64 bits the hardware keeps -- against the true 128-bit product."""
import os
import random
import re

import pytest

M32, M64 = 2**32 - 1, 2**64 - 1
PRIMES = (0xEC99BF0D8372CAAB, 0x82434FE90EDCEF39, 0xD4F06DB99D67BE4B, 0xBD9CACC22C6E9571,
          0x9C06FAF4D023E3AB, 0xC060724A8424F345, 0xCB5AF53AE3AAAC31)
P1, P2, P3 = PRIMES[1], PRIMES[2], PRIMES[3]
CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "hyper-gen_amd", "csrc")


def unit_text():
    """the text of the k-mer translation unit: hg_kmer_kernels.hip and the hg_kmer_*.h it includes"""
    top = open(os.path.join(CSRC, "hg_kmer_kernels.hip")).read()
    parts = re.findall(r'#include "(hg_kmer_\w+\.h)"', top)
    assert parts, "hg_kmer_kernels.hip includes its hg_kmer_*.h parts"
    return top + "".join(open(os.path.join(CSRC, p)).read() for p in parts)


def worst_cross_sum(P):
    """the predicate's left-hand side: the cross sum at x0 = x1 = 2^32 - 1"""
    p0, p1 = P & M32, P >> 32
    return M32 * p1 + M32 * p0 + ((M32 * p0) >> 32)


def cross_fits(P):
    return worst_cross_sum(P) < 2**64


def nocarry_sequence(x, P, addend):
    """HG_KS_MUL128_NC: -> (lo64(x P), hi64(x P) + addend) as the registers hold them"""
    x0, x1, p0, p1 = x & M32, x >> 32, P & M32, P >> 32
    a = (x0 * p0 + 0) & M64                     # v_mad_u64_u32 v[74:75], junk, XLO, PLO, 0
    z = (a >> 32) & M32                         # v_mov_b32 v68, v75        (v69 is 0: Z = {v68, 0})
    t = (x1 * p0 + z) & M64                     # v_mad_u64_u32 v[76:77], junk, XHI, PLO, v[68:69]
    t = (x0 * p1 + t) & M64                     # v_mad_u64_u32 v[76:77], junk, XLO, PHI, v[76:77]   (carry-out dropped)
    out = ((t >> 32) * 1 + addend) & M64        # v_mad_u64_u32 OUT, junk, v77, 1, ADDEND
    out = (x1 * p1 + out) & M64                 # v_mad_u64_u32 OUT, junk, XHI, PHI, OUT
    return (a & M32) | ((t & M32) << 32), out   # lo64 = {v74, v76}


def true_product(x, P, addend):
    m = x * P
    return m & M64, ((m >> 64) + addend) & M64


def test_primes_are_the_kernels():
    text = unit_text()
    found = {int(i): int(v, 16) for i, v in re.findall(r"constexpr uint64_t P(\d) = (0x[0-9A-Fa-f]+)ull;", text)}
    assert found == dict(enumerate(PRIMES))


def test_predicate_table():
    # prime: (p0 + p1, largest W / 2^64 to three places, carry possible)
    want = {1: (0x091203F22, 0.567, False), 3: (0x0EA0B4233, 0.914, False), 2: (0x172582C04, 1.447, True),
            4: (0x16C2ADE9F, 1.423, True), 5: (0x14485658F, 1.268, True)}
    for i, (psum, ratio, carry) in want.items():
        P = PRIMES[i]
        assert (P & M32) + (P >> 32) == psum, i
        assert round(worst_cross_sum(P) / 2**64, 3) == ratio, i
        assert cross_fits(P) == (not carry), i
    assert [cross_fits(P) for P in PRIMES] == [False, True, False, True, False, False, False]
    for P in PRIMES:  # the worst case is (2^32 - 1) (p0 + p1) + p0 - 1; p0 + p1 < 2^32 is sufficient for it to fit
        p0, p1 = P & M32, P >> 32
        assert worst_cross_sum(P) == M32 * (p0 + p1) + p0 - 1
        if p0 + p1 < 2**32:
            assert cross_fits(P)


EDGE = (0, 1, 2**31, 2**32 - 2, 2**32 - 1)
ADDENDS = (0, 1, 2**32 - 1, 2**32, 2**64 - 1)


@pytest.mark.parametrize("P", [P1, P3], ids=["P1", "P3"])
def test_sequence_at_the_edges(P):
    for x0 in EDGE:
        for x1 in EDGE:
            for addend in ADDENDS:
                x = x0 | (x1 << 32)
                assert nocarry_sequence(x, P, addend) == true_product(x, P, addend), (hex(x), hex(addend))


@pytest.mark.parametrize("P", [P1, P3], ids=["P1", "P3"])
def test_sequence_random(P):
    rng = random.Random(0x7A1 ^ P)
    for _ in range(100_000):
        x, addend = rng.getrandbits(64), rng.getrandbits(64)
        if nocarry_sequence(x, P, addend) != true_product(x, P, addend):
            pytest.fail("x = %#x, addend = %#x" % (x, addend))


def test_a_lost_carry_is_seen():
    """P2 does not fit: the sequence without the carry op is wrong there, and this test's arithmetic shows it"""
    x = 2**64 - 1
    got, want = nocarry_sequence(x, P2, 0), true_product(x, P2, 0)
    assert got != want
    assert got[0] == want[0] and (want[1] - got[1]) & M64 == 2**32  # the low half is right; the carry is bit 32 of the high half
