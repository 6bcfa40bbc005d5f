"""The two payload layouts of a .sketch file's hypervectors, stated on Python integers: a third formulation beside
oracle/hg_oracle.c and hyper-gen_amd/csrc/hg_formats.cpp, shared with neither (test_oracle.py checks the oracle against it,
test_gpu_bits_census.py the device's decoder)."""
import numpy as np


def bp8x_model(values, q):
    """BitPacker8x block from the crate's definition, bit by bit in Python integers: lane l = i % 8 owns a stream of 32*q
    bits, element r = i // 8 starts at bit r*q; an unmasked element spills up to bit 31 of its first word and, if it
    straddles a word boundary, its bits from (32 - c) upwards continue at bit 0 of the next word; word w of lane l = output
    u32 8w + l."""
    words = [[0] * 8 for _ in range(q)]
    for i, v in enumerate(values):
        lane, p = i % 8, (i // 8) * q
        w0, c = divmod(p, 32)
        words[w0][lane] |= (v << c) & 0xFFFFFFFF
        if c + q > 32:
            words[w0 + 1][lane] |= v >> (32 - c)
    return np.array(words, dtype="<u4").tobytes()


def naive_model(hv, q):
    """the non-AVX2 layout (src/hd.rs:158-166), on Python integers: the stream is the concatenation of the values' low q
    bits, LSB first; 16 stream bits per i16 word, (q*d + 16) // 16 words"""
    bits = []
    for x in hv:
        bits += [((int(x) & 0xFFFF) >> k) & 1 for k in range(q)]
    words = [0] * ((q * len(hv) + 16) // 16)
    for i, b in enumerate(bits):
        words[i // 16] |= b << (i % 16)
    return np.array(words, np.uint16).view(np.int16)
