"""The k-mer kernel's first t1ha2 mixup on bounded operands (HG_KS_MUL128_BOUNDED in hg_kmer_asm.h), in Python integers.

The stage computes lo64 and s + hi64 of ((s + w0) mod 2^64) * P, where w0 is the k-mer's first eight bytes -- each one of
"ACGT" -- and s is wave-uniform: the seed with P3 (k = 17..24, seeds below 2^28 only) or the length K with P4 (k = 25..32).
The bounded text replaces a 64-bit add, a "x 1" product and a carry add by two 32-bit adds.  Here every instruction of it is
restated with its register width, every intermediate is checked against the bound the text relies on, and the results are
compared with the plain 128-bit product."""
import os
import random
import re

import pytest

P3 = 0xBD9CACC22C6E9571
P4 = 0x9C06FAF4D023E3AB
M32, M64 = (1 << 32) - 1, (1 << 64) - 1
SEED_END = 1 << 28

CASES = [(P3, s) for s in (0, 1, 123, SEED_END - 1)] + [(P4, k) for k in range(25, 33)]
IDS = ["P3-seed%d" % s for s in (0, 1, 123, SEED_END - 1)] + ["P4-K%d" % k for k in range(25, 33)]


def acgt_words():
    rng = random.Random(20240611)
    words = [int.from_bytes(b"T" * 8, "little"), int.from_bytes(b"A" * 8, "little")]
    words += [int.from_bytes(bytes(rng.choice(b"ACGT") for _ in range(8)), "little") for _ in range(4000)]
    return words


WORDS = acgt_words()


def reference(w0, s, P):
    """(lo64, s + hi64 mod 2^64) of mixup64's product"""
    m = ((s + w0) & M64) * P
    return m & M64, (s + (m >> 64)) & M64


def bounded_stage(w0l, w0h, s, P):
    """the bounded text, one line per instruction; asserts: what each instruction's width takes for granted"""
    p0, p1 = P & M32, P >> 32
    x0 = w0l + s                      # v_add_u32 v72, s, W0.lo
    assert x0 <= M32, "carry out of the low dword of s + w0"
    a = x0 * p0                       # v_mad_u64_u32 v[74:75], x0, p0, 0
    z = a >> 32                       # v_mov_b32 v68, v75       (Z = {hi32(A), 0})
    t = w0h * p0 + z                  # v_mad_u64_u32 v[76:77], W0.hi, p0, Z
    assert t <= M64
    w = x0 * p1 + t                   # v_mad_u64_u32 v[76:77], x0, p1, v[76:77]   (its carry-out is dropped)
    assert w <= M64, "carry out of the third product"
    z = (w >> 32) + s                 # v_add_u32 v68, s, v77
    assert z <= M32, "hi32(W) + s wraps 32 bits"
    out = w0h * p1 + z                # v_mad_u64_u32 OUT, W0.hi, p1, Z
    assert out <= M64, "s + hi64 wraps 64 bits"
    return ((w & M32) << 32) | (a & M32), out


@pytest.mark.parametrize("P,s", CASES, ids=IDS)
def test_bounded_stage_equals_the_128_bit_product(P, s):
    for w0 in WORDS:
        assert bounded_stage(w0 & M32, w0 >> 32, s, P) == reference(w0, s, P), hex(w0)


@pytest.mark.parametrize("P,s", CASES, ids=IDS)
def test_worst_case_is_the_largest_operands(P, s):
    """every intermediate grows with x0, x1 and s: the all-T word with the case's s bounds every ACGT word"""
    p0, p1 = P & M32, P >> 32
    x1 = 0x54545454
    x0 = x1 + s
    assert x0 <= M32
    w = x0 * p1 + x1 * p0 + ((x0 * p0) >> 32)
    assert w <= M64 and (w >> 32) + s <= M32 and x1 * p1 + (w >> 32) + s <= M64
    assert all((w0 & M32) <= x1 and (w0 >> 32) <= x1 for w0 in WORDS)


def test_seed_limit_has_margin_and_the_general_text_is_needed_beyond():
    """the P3 bounds hold up to 0x66C7395F (hi32(W) + seed wraps first) -- 2^28 is well inside; a seed of 2^32 or more has a
    high dword the 32-bit add does not see, so such seeds must take the general text"""
    t = int.from_bytes(b"T" * 8, "little")
    assert bounded_stage(t & M32, t >> 32, 0x66C7395F, P3) == reference(t, 0x66C7395F, P3)
    with pytest.raises(AssertionError):
        bounded_stage(t & M32, t >> 32, 0x66C73960, P3)
    assert SEED_END - 1 < 0x66C7395F
    s = (1 << 32) + 5
    p0, p1 = P3 & M32, P3 >> 32
    x0 = ((t & M32) + s) & M32  # what the 32-bit add would produce
    lo_wrong = (x0 * p0) & M32
    assert lo_wrong == reference(t, s, P3)[0] & M32  # the low dword alone agrees ...
    assert ((x0 | ((t >> 32) << 32)) * P3) & M64 != reference(t, s, P3)[0]  # ... the product does not


def test_source_uses_the_limit_checked_here():
    csrc = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "hyper-gen_amd", "csrc")
    text = open(os.path.join(csrc, "hg_kmer_kernels.hip")).read()  # the translation unit: the .hip and the hg_kmer_*.h it includes
    parts = re.findall(r'#include "(hg_kmer_\w+\.h)"', text)
    assert parts
    text += "".join(open(os.path.join(csrc, p)).read() for p in parts)
    m = re.search(r"FIRST_SEED_END\s*=\s*1ull\s*<<\s*(\d+)", text)
    assert m and (1 << int(m.group(1))) == SEED_END
    assert "seed < FIRST_SEED_END" in text and "first_mixup_bounded(P3, FIRST_SEED_END - 1)" in text
