"""One row per compiled clustering, tree and statistics kernel of libhypergen_hip.so -- single linkage and the finishing
kernels every scheme shares (cluster_*), the greedy and set-cover representative schemes, the single-linkage tree, average
and complete linkage, the cluster statistics and neighbour joining -- and how an input reaches it.

test_cluster_census.py (CPU) checks that the names here are exactly the instantiations the built library holds: a kernel
added without a row, or a row whose kernel is gone, fails there.  test_gpu_cluster_census.py (GPU) runs every row's entry at a
small input against the Python models (tests/cluster_*_ref.py, nj_ref.py), with the input the row names.

A row's name is spelled as rocprofv3 spells it.  Its route:
* entry: the C entry point (without its hg_ prefix) that queues the kernel: the _dev, _hits_dev or _matrix_dev form that
  takes device pointers;
* debug: the hg_ctx_set_debug keys the call runs under (pair_limit: row blocks of the symmetric comparison from that many
  pairs on); none: the library chooses;
* inputs: what the input has to be for the kernel to run, or -- for a kernel every call launches -- for its work to show in
  the result;
* unreachable: None, or why no input reaches the kernel (printed by the CPU test).
"""
from collections import namedtuple

Row = namedtuple("Row", "name entry debug inputs unreachable")

ROUNDS = "ani_th is no NaN and <= 100: the rounds run"
EMIT = "one of d_into, d_level, d_size given"

CLUSTER_ROWS = [
    Row("cluster_init_kernel", "cluster_init_dev", {}, "n >= 1", None),
    Row("cluster_hook_kernel", "cluster_add_hits_dev", {}, "n_hits >= 1", None),
    # the finishing kernels of all six schemes, on tiles of 1024 nodes (compress, root_ids) and chunks of 256 tiles (scan)
    Row("cluster_compress_kernel", "cluster_finish_dev", {}, "n >= 1; paths of depth > 1: hits hooked in several calls", None),
    Row("cluster_scan_tiles_kernel", "cluster_finish_dev", {}, "always (n = 0: the count is 0); roots in more than one tile", None),
    Row("cluster_root_ids_kernel", "cluster_finish_dev", {}, "n >= 1; roots on both sides of a tile border", None),
    Row("cluster_member_ids_kernel", "cluster_finish_dev", {}, "n >= 1; a member whose root sits in another tile", None),
    # rep / ani of the representative schemes (greedy and set cover): a member's ANI shows only with d_ani
    Row("cluster_rep_ani_kernel", "cluster_greedy_hits_dev", {}, "n >= 1; d_ani given and a member present", None),
]
GREEDY_ROWS = [
    Row("greedy_init_kernel", "cluster_greedy_hits_dev", {}, "n >= 1", None),
    # every block enters; the kernel's member branch needs a node that a representative of an EARLIER row block covers
    Row("greedy_enter_kernel", "cluster_greedy_dev", {"pair_limit": "small"}, "several row blocks, a member in a later one", None),
    Row("greedy_mark_kernel", "cluster_greedy_hits_dev", {}, "a chain i - i + 1 - i + 2: the blocked mark, several rounds", None),
    Row("greedy_decide_kernel", "cluster_greedy_hits_dev", {}, "n >= 1", None),
    Row("greedy_assign_kernel", "cluster_greedy_hits_dev", {}, "a member with two representatives: the higher ANI wins", None),
]
SETCOVER_ROWS = [
    Row("setcover_init_kernel", "cluster_setcover_hits_dev", {}, "n >= 1", None),
    Row("setcover_count_kernel", "cluster_setcover_hits_dev", {}, "nodes of different degree", None),
    Row("setcover_spread_kernel", "cluster_setcover_hits_dev", {}, "two candidates two hops apart (both of its launches: m1, m2)", None),
    Row("setcover_select_kernel", "cluster_setcover_hits_dev", {}, "n >= 1", None),
    Row("setcover_cover_kernel", "cluster_setcover_hits_dev", {}, "a pair given twice with two ANI values", None),
    Row("setcover_settle_kernel", "cluster_setcover_hits_dev", {}, "a path: several rounds", None),
]
TREE_ROWS = [
    Row("tree_init_kernel", "cluster_tree_hits_dev", {}, "n >= 1", None),
    Row("tree_best_ani_kernel", "cluster_tree_hits_dev", {}, "n_hits >= 1", None),
    Row("tree_best_pair_kernel", "cluster_tree_hits_dev", {}, "n_hits >= 1; ties of the best ANI: the smallest pair wins", None),
    Row("tree_select_kernel", "cluster_tree_hits_dev", {}, "n_hits >= 1; a mutual selection is emitted once", None),
    Row("tree_hook_kernel", "cluster_tree_hits_dev", {}, "n_hits >= 1", None),
    Row("tree_compress_kernel", "cluster_tree_hits_dev", {}, "n_hits >= 1; several rounds", None),
]
AVERAGE_ROWS = [
    Row("average_init_kernel", "cluster_average_matrix_dev", {}, "n >= 1", None),
    Row("average_fill_kernel", "cluster_average_matrix_dev", {}, "n >= 1", None),
    # the lower triangle the rounds read is the mirror's: a caller's lower triangle of NaN must not show
    Row("average_mirror_kernel", "cluster_average_matrix_dev", {}, "n >= 2, more than one mirror tile; garbage below the diagonal", None),
    Row("average_best_kernel", "cluster_average_matrix_dev", {}, ROUNDS, None),
    Row("average_pair_kernel", "cluster_average_matrix_dev", {}, ROUNDS, None),
    Row("average_rows_kernel", "cluster_average_matrix_dev", {}, ROUNDS + "; a merge", None),
    Row("average_cols_kernel", "cluster_average_matrix_dev", {}, ROUNDS + "; a merge", None),
    Row("average_emit_kernel", "cluster_average_matrix_dev", {}, EMIT, None),
]
COMPLETE_ROWS = [
    Row("complete_init_kernel", "cluster_complete_matrix_dev", {}, "n >= 1", None),
    Row("complete_fill_kernel", "cluster_complete_matrix_dev", {}, "n >= 1", None),
    Row("complete_mirror_kernel", "cluster_complete_matrix_dev", {}, "n >= 2, more than one mirror tile; garbage below the diagonal", None),
    # from round 2 on only the rows a merge invalidated are scanned again: the rescan needs three rounds or more
    Row("complete_best_kernel", "cluster_complete_matrix_dev", {}, ROUNDS + "; three rounds or more: the rescan of invalidated rows", None),
    Row("complete_pair_kernel", "cluster_complete_matrix_dev", {}, ROUNDS, None),
    Row("complete_rows_kernel", "cluster_complete_matrix_dev", {}, ROUNDS + "; a merge", None),
    Row("complete_cols_kernel", "cluster_complete_matrix_dev", {}, ROUNDS + "; a merge", None),
    Row("complete_emit_kernel", "cluster_complete_matrix_dev", {}, EMIT, None),
]
STATS_ROWS = [
    Row("cluster_stats_check_kernel", "cluster_stats_matrix_dev", {}, "n >= 1", None),
    Row("cluster_stats_rows_kernel", "cluster_stats_matrix_dev", {}, "n >= 1", None),
    Row("cluster_stats_fold_kernel", "cluster_stats_matrix_dev", {}, "d_stat given", None),
    Row("cluster_stats_medoid_kernel", "cluster_stats_matrix_dev", {}, "d_stat given", None),
    Row("cluster_stats_emit_kernel", "cluster_stats_matrix_dev", {}, "d_stat given and n_clusters >= 1 (also n = 0: empty records)", None),
]
NJ_ROWS = [
    Row("nj_init_kernel", "nj_matrix_dev", {}, "n >= 2", None),
    Row("nj_fill_kernel", "nj_matrix_dev", {}, "n >= 2", None),
    Row("nj_mirror_kernel", "nj_matrix_dev", {}, "n >= 2, more than one mirror tile; garbage below the diagonal", None),
    Row("nj_rsum_kernel", "nj_matrix_dev", {}, "n >= 2", None),
    Row("nj_best_kernel", "nj_matrix_dev", {}, "n >= 2", None),
    Row("nj_pick_kernel", "nj_matrix_dev", {}, "n >= 2", None),
    Row("nj_update_kernel", "nj_matrix_dev", {}, "n >= 3: every join but the last", None),
]
FAMILY_ROWS = {"cluster": CLUSTER_ROWS, "greedy": GREEDY_ROWS, "setcover": SETCOVER_ROWS, "tree": TREE_ROWS, "average": AVERAGE_ROWS,
               "complete": COMPLETE_ROWS, "cluster_stats": STATS_ROWS, "nj": NJ_ROWS}
ROWS = [r for rows in FAMILY_ROWS.values() for r in rows]
