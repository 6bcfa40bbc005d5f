"""One row per compiled kernel of libhypergen_frag.so and how an input reaches it.  Neither kernel is a template: a reduction is
frag_best_kernel over every block of the matrix, then frag_fold_kernel over the genomes whose bests are complete, in the order
of the rows.

test_frag_census.py (CPU) checks that the names here are exactly the kernels `nm -C` finds in the built library and the ones
hg_frag_kernel_names() lists.  test_gpu_frag_matrix.py (GPU) checks through hg_frag_launch_counts() that its cases have launched
every row.

A row: the name as rocprofv3 spells it, the entry points that reach it, what it does.  A comparison without rows or columns
stops in front of frag_best_kernel; hg_frag_sketch_seq_dev launches neither (its kernels are libhypergen_hip.so's).
"""
from collections import namedtuple

Row = namedtuple("Row", "name entries what")

REDUCE = ("hg_frag_ani_matrix_dev", "hg_frag_ani_dev", "hg_frag_ani")
ROWS = [
    Row("frag_best_kernel", REDUCE, "32 rows of one reference genome x 256 columns per wave -> 64-bit max into the table of bests"),
    Row("frag_fold_kernel", REDUCE, "one workgroup per (reference genome, query genome): matched, sum, total; the bests as records"),
]
