"""One row per compiled kernel of libhypergen_rec.so and how an input reaches it.  None of the kernels is a template: a split is
the same eight launches for every text, in the order of the rows.

test_rec_census.py (CPU) checks that the names here are exactly the kernels `nm -C` finds in the built library and the ones
hg_rec_kernel_names() lists.  test_gpu_rec.py (GPU) checks through hg_rec_launch_counts() that its cases have launched every row.

A row: the name as rocprofv3 spells it, the entry points that reach it, what it does.  hg_rec_count_dev stops in front of the
scatter; a text without a header line stops in front of the per-record kernels.
"""
from collections import namedtuple

Row = namedtuple("Row", "name entries what")

COUNT = ("hg_rec_count_dev", "hg_rec_split_dev", "hg_rec_split", "hg_rec_sketch_text_dev")
SPLIT = COUNT[1:]
ROWS = [
    Row("rec_block_summary_kernel", COUNT, "4096 bytes of text per workgroup -> the block's summary"),
    Row("rec_tile_reduce_kernel", COUNT, "1024 block summaries -> the tile's summary"),
    Row("rec_block_prefix_kernel", COUNT, "every block's exclusive prefix, the text's totals"),
    Row("rec_mark_kernel", COUNT, "per header line: hdr_off, hdr_len, id_len, sequence bytes in front of it"),
    Row("rec_pad_reduce_kernel", COUNT, "2048 records -> the sum of their pads"),
    Row("rec_pad_scan_kernel", COUNT, "exclusive scan of the tile sums"),
    Row("rec_offsets_kernel", COUNT, "per record: seq_off, seq_len"),
    Row("rec_scatter_kernel", SPLIT, "sequence bytes and 'N' pads into the layout"),
]
