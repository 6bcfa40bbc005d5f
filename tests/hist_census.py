"""One row per compiled kernel of libhypergen_hist.so and how an input reaches it.  The one kernel is no template: the copies of
the LDS table, the slices of the bin range and the selection are run-time arguments of hist_count_kernel, and a block of the
matrix is one launch of it per 32 768 row tiles.

test_hist_census.py (CPU) checks that the names here are exactly the kernels `nm -C` finds in the built library and the ones
hg_hist_kernel_names() lists.  test_gpu_hist_matrix.py (GPU) checks through hg_hist_launch_counts() that its cases have launched
every row.

A row: the name as rocprofv3 spells it, the entry points that reach it, what it does.  A block without rows or columns, and one
that lies wholly outside the selection, stops in front of the kernel.
"""
from collections import namedtuple

Row = namedtuple("Row", "name entries what")

COUNT = ("hg_hist_add_matrix_dev", "hg_hist_dev", "hg_hist")
ROWS = [
    Row("hist_count_kernel", COUNT, "256 rows x 256 columns x one slice of the bins per workgroup: bin 0 in registers, the rest by LDS "
                                    "atomics, the non-zero counters by 64-bit adds into the table"),
]
