"""One row per compiled support kernel of libhypergen_hip.so -- the kernels that order and cut hit lists (hg_hits.hip), select
the top N of a search (hg_search.hip), prepare and judge the operands of the dist GEMMs (hg_dist_prep.h), and the four small
ones around them (listed pairs, logf, ANI from dots, the publishing of result words) -- and how an input reaches it.  Their
names match no family of kernel_census.py, set_encode_census.py, min_count_census.py or bits_census.py.

test_select_census.py (CPU) checks that the names here are exactly the instantiations the built library holds: a kernel added
without a row, or a row whose kernel is gone, fails there.  test_gpu_select_census.py (GPU) runs every row at one small input
and the sorts, the top-k cut, the search and the global indices of the block calls at the shapes where a border decides.

A row's name is spelled as rocprofv3 spells it.  Its route:
* entry: "sort_hits" (hg_sort_ani_hits_dev), "topk" (hg_topk_per_query_dev), "tree_edges" (hg_sort_tree_edges_dev, through
  hg_cluster_tree_hits_dev), "search" (hg_search_topk_block_dev), "dist" (hg_dist_dev), "dist_ops" (hg_dist_prep_ops_dev +
  hg_dist_block_ops_dev), "pairs" (hg_ani_pairs_dev), "logf" (hg_logf_dev), "ani_from_dots" (hg_ani_from_dots_dev) or "publish"
  (any call that reads result words back: hg_cluster_finish_dev is the smallest);
* debug: the hg_ctx_set_debug keys the call runs under (dist_path: the operand form whose prepass the row is); none: the
  library chooses;
* inputs: what the input has to be for the kernel to run (the input classes of test_gpu_kernel_census.py for the prepass
  rows; the sort rows: which pass of which entry launches them);
* unreachable: None, or why no input reaches the kernel (printed by the CPU test).
"""
from collections import namedtuple

Row = namedtuple("Row", "name entry debug inputs unreachable")

ENTRIES = ("sort_hits", "topk", "tree_edges", "search", "dist", "dist_ops", "pairs", "logf", "ani_from_dots", "publish")

HITS_ROWS = [
    # gather_keys_kernel<WHAT>: the key of one LSD pass.  0 = ref * Q + qry (u64), 1 = the ANI's bits, 2 = ref, 3 = qry,
    # 4 = the ANI's order-preserving key of any sign
    Row("gather_keys_kernel<0>", "sort_hits", {}, "pass 1: the enumeration key", None),
    Row("gather_keys_kernel<1>", "sort_hits", {}, "pass 2: ANI bits (also topk's second pass)", None),
    Row("gather_keys_kernel<2>", "topk", {}, "pass 1: reference index (also tree_edges' second pass)", None),
    Row("gather_keys_kernel<3>", "topk", {}, "pass 3: query index (also tree_edges' first pass)", None),
    Row("gather_keys_kernel<4>", "tree_edges", {}, "pass 3: ANI key, negative values and both zeros included", None),
    Row("permute_hits_kernel", "sort_hits", {}, "n >= 2", None),
    Row("topk_kernel", "topk", {}, "n >= 1", None),
    Row("fill_empty_kernel", "topk", {}, "Q * k >= 1", None),
    # radix_*_kernel<K, DESC>: one histogram, one row scan and one stable scatter per 8-bit digit
    Row("radix_hist_kernel<unsigned int, false>", "topk", {}, "ascending u32 passes: ref, qry", None),
    Row("radix_hist_kernel<unsigned int, true>", "sort_hits", {}, "descending u32 passes: ANI", None),
    Row("radix_hist_kernel<unsigned long, true>", "sort_hits", {}, "descending u64 passes: the enumeration key", None),
    Row("radix_scan_kernel", "sort_hits", {}, "every pass; its second chunk: n > 1 048 576 (more than 256 tiles)", None),
    Row("radix_scatter_kernel<unsigned int, false>", "topk", {}, "ascending u32 passes: ref, qry", None),
    Row("radix_scatter_kernel<unsigned int, true>", "sort_hits", {}, "descending u32 passes: ANI", None),
    Row("radix_scatter_kernel<unsigned long, true>", "sort_hits", {}, "descending u64 passes: the enumeration key", None),
]
SEARCH_ROWS = [
    Row("search_topk_select_kernel", "search", {}, "R >= 1", None),
    Row("search_topk_merge_kernel", "search", {}, "R >= 1", None),
    Row("search_topk_emit_kernel", "search", {}, "Q * k >= 1 (also R = 0)", None),
]
PREP_ROWS = [
    # the raw-value chain (f16 copies of the values): the fast prepass and, on a thresholded call, its verdict on the device;
    # the every-window prepass when neither the whole row nor the 2 048- / 1 024-dim windows are safe (the rerun classes).
    # Borders: test_gpu_dist_boundaries.py
    Row("prep_fast_kernel", "dist", {"dist_path": "f16"}, "sketch", None),
    Row("decide_kernel", "dist", {"dist_path": "f16"}, "sketch", None),
    Row("prep_kernel", "dist", {"dist_path": "f16"}, "r512", None),
    # centred f16 operands and byte operands.  Borders: test_gpu_dist_boundaries.py
    Row("prep_cen_kernel", "dist", {"dist_path": "cen"}, "sketch", None),
    Row("decide_cen_kernel", "dist", {"dist_path": "cen"}, "sketch", None),
    Row("prep_i8_kernel", "dist", {"dist_path": "i8"}, "sketch", None),
    # prepared byte operands: the reference side's control records are unpacked in the place of its prepass.
    # Borders: test_gpu_dist_ops.py
    Row("unpack_meta_kernel", "dist_ops", {}, "sketch", None),
]
OTHER_ROWS = [
    Row("ani_pairs_kernel", "pairs", {}, "n_pairs >= 1 (borders: test_gpu_ani_pairs.py)", None),
    Row("logf_kernel", "logf", {}, "n >= 1 (every float in (0, 1]: test_gpu_ani_exact.py)", None),
    Row("ani_from_dots_kernel", "ani_from_dots", {}, "n >= 1 (borders: test_gpu_ani_exact.py)", None),
    Row("publish_words_kernel", "publish", {}, "result words read back", None),
]
ROWS = HITS_ROWS + SEARCH_ROWS + PREP_ROWS + OTHER_ROWS
