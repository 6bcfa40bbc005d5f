"""The texts the record splitter is tested on, in one place so that the CPU tests (hg_rec_split_host) and the GPU tests
(hg_rec_count_dev, hg_rec_split_dev) run the same ones.  B is hg_rec_block_bytes(): the bytes of text one workgroup reads, so
that bytes can be placed on a block boundary.  No text is longer than about 4 B.  What a text must give is tests/rec_ref.py's
word; a text with sequence data before its first header is a case like any other (rec_ref raises, the library says HG_ERR_IO)."""
import numpy as np

ANCHOR = b">seq1 first record\nACGTACGTAC\nGGTTAACC\n>seq2\nTTTT\nAC\n>seq3\tthird\r\nGATTACA\r\nGA\r\n"
MOTIF = b"GG\n>id desc\r\nACGT\r\nAC\n"
ALPHABET = np.frombuffer(b">\n\rAcN \t", np.uint8)


def filler(length):
    """a record of exactly `length` bytes of text whose last line is an open sequence line (length >= 4)"""
    assert length >= 4
    return b">f\n" + b"A" * (length - 3)


def cases(B):
    out = []

    def add(name, text):
        out.append((name, bytes(text)))

    # 1. the anchor: three records with wrapped lines
    add("anchor", ANCHOR)
    # 2. the motif, slid: byte i of it is the last byte of block 0 and byte i + 1 the first of block 1 (i = -1: the motif starts
    #    block 1), among them "\r | \n", "\n | >" and "> | i"
    for i in range(-1, len(MOTIF)):
        add("motif_%02d" % (i + 1), filler(B - 1 - i) + MOTIF + b">t\nTT\n")
    #    a '>' that is the first byte of a block while the block before did not end in LF: a sequence byte
    add("gt_inside_line_at_block_start", filler(B) + b">A>C\nGG\n>t\n>TT\n")
    #    ... and one behind an LF that ends the block: a header
    add("gt_behind_lf_at_block_start", filler(B - 1) + b"\n>h>h x\nGG\n")
    # 3. long lines: a header line of 2.5 B (its identifier ends after 2 B, or nowhere), a sequence line of 3 B + 1 bytes without
    #    LF; blocks without any LF in both states
    add("header_2p5B_blank", b">s\nAC\n>" + b"h" * (2 * B) + b" " + b"d" * (B // 2) + b"\nACGT\n>x y\nAC\n")
    add("header_2p5B_no_blank", b">" + b"h" * (5 * B // 2) + b"\r\nACGT\n>x\nAC\n")
    add("header_2p5B_unterminated", b">s\nACG\n>" + b"h" * (5 * B // 2))
    add("sequence_3B_plus_1_unterminated", b">s d\n" + b"ACGT" * (3 * B // 4) + b"A")
    add("sequence_3B_then_more", b">s\n" + b"ACGT" * (3 * B // 4) + b"\nGG\n>t\nT\n")
    # 4. dense tiny records: more headers in a block than it has lanes; empty records and empty identifiers
    add("dense_a", b">a\nA\n" * (2 * B // 5 + 3))
    add("dense_empty", b">\n>\n" * (B // 2))
    add("dense_mixed", (b">\n>b c\nAC\n>\n\n>d\nA\nC\nG\n") * (2 * B // 22 + 1))
    # 5. record lengths 0 to 9: offsets and pads
    add("lengths_0_to_9", b"".join(b">r%d\n" % k + (b"ACGTACGTAC"[:k] + b"\n" if k else b"") for k in range(10)))
    add("lengths_9_to_0_split", b"".join(b">r%d\n" % k + b"".join(b"ACGTACGTAC"[j:j + 1] + b"\n" for j in range(k)) for k in range(9, -1, -1)))
    # 6. the ends of a text
    add("no_final_lf", b">a\nACGT\n>b\nACG")
    add("final_cr", b">a\nACGT\n>b\nACG\r")
    add("final_header_without_lf", b">a\nACGT\n>last one")
    add("final_header_with_cr", b">a\nACGT\n>last\r")
    add("final_crlf", b">a\nACGT\r\n")
    add("cr_inside_lines", b">a\rb\r\r\nAC\rGT\r\r\n\rA\n")
    add("empty", b"")
    add("lfs_only", b"\n" * 7)
    add("one_header_byte", b">")
    for n in (B - 1, B, B + 1):
        add("n_%d_open" % n, b">e\n" + b"A" * (n - 3))
        add("n_%d_lf" % n, b">e\n" + b"A" * (n - 4) + b"\n")
        add("n_%d_crlf_header" % n, b">e\nAC\n>" + b"h" * (n - 9) + b"\r\n")
    # 8. in front of the first header: sequence data is an error, empty lines are not
    add("sequence_before_header", b"ACGT\n>a\nAC\n")
    add("fastq", b"@r1\nACGT\n+\nIIII\n")
    add("blank_before_header", b" \n>a\nAC\n")
    add("cr_content_before_header", b"\r\r\n>a\nAC\n")
    add("only_sequence", b"A")
    add("sequence_a_block_before_header", b"A" + b"\n" * B + b">a\nC\n")
    add("empty_lines_before_header", b"\n\r\n\n>a\nAC\n")
    add("empty_lines_a_block_before_header", b"\r\n" * (B // 2 + 1) + b">a x\nC\n")
    add("gt_inside_first_line", b"A>\n>a\nC\n")
    return out


def fuzz_texts(B, seed=20, count=200):
    """seeded random texts of 0 to 3 B bytes over '>', LF, CR, 'A', 'c', 'N', blank and tab.  Three in four start with '>', so
    that most of them are records and not the error; the weights of LF and '>' vary from text to text."""
    rng = np.random.default_rng(seed)
    out = []
    for t in range(count):
        n = int(rng.integers(0, 3 * B + 1)) if t % 8 else int(rng.integers(0, 40))
        w = np.array([rng.choice([0.02, 0.1, 0.3]), rng.choice([0.02, 0.1, 0.3]), rng.choice([0.0, 0.05, 0.2]), 0.3, 0.2, 0.05, 0.03, 0.02])
        text = rng.choice(ALPHABET, n, p=w / w.sum())
        if n and t % 4:
            text[0] = ord(">")
        out.append(text.tobytes())
    return out
