"""One row per compiled kernel of libhypergen_tx.so and how an input reaches it.  The library has one kernel template,
tx_kmer_sample_kernel<KW>: KW = ceil(k / 8) is the number of 8-byte words t1ha2 mixes for a k-mer of k residues; k itself is a
kernel argument.

test_tx_census.py (CPU) checks that the names here are exactly the instantiations `nm -C` finds in the built library.
test_gpu_tx.py (GPU) runs every row at both ends of its range of k -- the lengths at which the hash's tail word is one byte and
a whole word -- and ctx.last_kernel("kmer") names the row.

A row: the name as hg_ctx_last_kernel and rocprofv3 spell it, the entry points that reach it, the values of k it serves.
"""
from collections import namedtuple

Row = namedtuple("Row", "name entries ksizes")

ENTRIES = ("hg_tx_hash_sample", "hg_tx_sketch_batch_dev", "hg_tx_sketch_batch")
ROWS = [Row("tx_kmer_sample_kernel<%d>" % kw, ENTRIES, tuple(range(8 * kw - 7, 8 * kw + 1))) for kw in (1, 2, 3, 4)]
