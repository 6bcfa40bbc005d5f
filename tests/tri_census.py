"""One row per compiled kernel of libhypergen_tri.so and how an input reaches it.  The one kernel is no template: the layout is a
run-time argument of tri_format_kernel, and a block of the matrix is one launch of it per 32 768 row tiles.

test_tri_census.py (CPU) checks that the names here are exactly the kernels `nm -C` finds in the built library and the ones
hg_tri_kernel_names() lists.  test_gpu_tri_matrix.py (GPU) checks through hg_tri_launch_counts() that its cases have launched
every row.

A row: the name as rocprofv3 spells it, the entry points that reach it, what it does.  A block without rows or columns, and the
block of row 0 alone under HG_TRI_LOWER, stops in front of the kernel.
"""
from collections import namedtuple

Row = namedtuple("Row", "name entries what")

FORMAT = ("hg_tri_format_dev", "hg_tri_dev", "hg_tri_stream_dev", "hg_tri")
ROWS = [
    Row("tri_format_kernel", FORMAT, "32 rows x 256 columns per workgroup: 16 bytes of floats in and 32 bytes of text out per lane and row, "
                                     "the fields packed in registers, 16-byte stores where the row's alignment allows"),
]
