"""hyper-gen_amd -- ctypes binding of libhypergen_hip.so (include/hypergen.h).

This is a harness-side mirror of the C ABI: the product is the shared library (HIP kernels +
C ABI) and the C++ `hyper-gen` CLI next to it.  There is no CPU fallback here: if the
library is missing, or no HIP device is usable, calls raise.

Import it as `hypergen_amd` (see the shim at the repo root; the directory name carries a
hyphen because it is the reference's crate name).

Note for processes that also use PyTorch-ROCm: import torch BEFORE this module loads the library
(torch bundles its own copy of the HIP runtime; loaded second it finds no devices).
"""
import ctypes as C
import functools
import os
import threading
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = (os.environ.get("HYPERGEN_LIB") or None) or os.path.join(_HERE, "libhypergen_hip.so")  # override: development builds
CLI_PATH = os.path.join(_HERE, "hyper-gen")

LAYOUT_SCALAR, LAYOUT_AVX2 = 0, 1
GATHER_PEER, GATHER_RCCL = 0, 1
ANI_MASH, ANI_CONTAINMENT, ANI_MAX_CONTAINMENT = 0, 1, 2  # hg_ctx_set_ani_metric
PAIRS_MASH, PAIRS_CONTAINMENT, PAIRS_MAX_CONTAINMENT, PAIRS_CONTAINMENT_REF = 1, 2, 4, 8  # columns of hg_ani_pairs (HG_PAIRS_*)
PAIRS_EMPTY = 0xFFFFFFFF  # ref_idx of an empty slot in a pair list
NORM_ACGT, NORM_U2T = 0, 1
(OK, ERR_INVALID, ERR_NO_DEVICE, ERR_HIP, ERR_OOM, ERR_CAPACITY, ERR_UNSUPPORTED, ERR_IO,
 ERR_INEXACT) = range(9)


T_NAMES = ("kmer", "sort", "encode", "dist_prep", "dist")
T_COUNT = len(T_NAMES)


class HgError(RuntimeError):
    def __init__(self, status, msg):
        super().__init__("hypergen status %d: %s" % (status, msg))
        self.status = status


class SketchParams(C.Structure):
    _fields_ = [("ksize", C.c_uint32), ("canonical", C.c_uint32), ("scaled", C.c_uint64),
                ("seed", C.c_uint64), ("hv_d", C.c_uint32), ("hv_layout", C.c_uint32),
                ("norm_mode", C.c_uint32), ("min_count", C.c_uint32)]


class AniHit(C.Structure):
    _fields_ = [("ref_idx", C.c_uint32), ("qry_idx", C.c_uint32), ("ani", C.c_float)]


ANI_HIT_DTYPE = np.dtype([("ref_idx", "<u4"), ("qry_idx", "<u4"), ("ani", "<f4")])
HAM_HIT_DTYPE = np.dtype([("ref_idx", "<u4"), ("qry_idx", "<u4"), ("dist", "<u4")])


class FileSketch(C.Structure):
    _fields_ = [("ksize", C.c_uint8), ("canonical", C.c_uint8), ("hv_quant_bits", C.c_uint8),
                ("pad", C.c_uint8), ("hv_norm_2", C.c_int32), ("scaled", C.c_uint64),
                ("seed", C.c_uint64), ("hv_d", C.c_uint64), ("file_str", C.c_char_p),
                ("hv", C.POINTER(C.c_int16)), ("hv_len", C.c_uint64)]


EXPORTS = [
    "hg_status_str", "hg_last_error", "hg_version", "hg_ctx_create", "hg_ctx_destroy",
    "hg_ctx_set_stream", "hg_ctx_reset_stream", "hg_ctx_sync", "hg_ctx_sketch_step_counts", "hg_sketch_plan_describe", "hg_logf_dev", "hg_ani_from_dots_dev", "hg_device_count", "hg_dev_alloc", "hg_dev_free",
    "hg_copy_h2d", "hg_copy_d2h", "hg_sketch_params_default", "hg_kmer_hash_sample",
    "hg_kmer_hash_sample_min_count",
    "hg_hv_encode", "hg_sketch_batch_dev", "hg_sketch_batch", "hg_dist_full", "hg_dist_full_dev",
    "hg_dist", "hg_dist_dev", "hg_sort_ani_hits", "hg_hv_quant_bits", "hg_hv_pack", "hg_hv_packed_bytes",
    "hg_hv_unpack", "hg_sketch_file_write", "hg_sketch_file_read", "hg_sketch_file_count",
    "hg_sketch_file_get", "hg_sketch_file_free", "hg_read_merge_seq", "hg_read_merge_seq_into", "hg_free",
    "hg_synth_genomes_dev", "hg_ctx_enable_timing", "hg_ctx_timings", "hg_ctx_last_kernel",
    "hg_hv_binarize_dev", "hg_hamming_full_dev", "hg_hamming_search_dev",
    "hg_ctx_set_debug", "hg_read_fastx_into", "hg_dist_block_dev", "hg_hamming_search_block_dev",
    "hg_multi_create", "hg_multi_destroy", "hg_multi_size", "hg_multi_ctx", "hg_multi_last_error", "hg_shard_range",
    "hg_multi_peer_report", "hg_multi_set_gather", "hg_multi_gather_mode", "hg_multi_gather_report",
    "hg_sketch_batch_multi", "hg_dist_multi", "hg_dist_multi_dev", "hg_hamming_search_multi",
    "hg_sort_ani_hits_dev", "hg_sort_ani_hits_staged", "hg_topk_per_query_dev", "hg_ctx_last_dist_path",
    "hg_ctx_last_hamming_path", "hg_read_fastx_pinned", "hg_pinned_free",
    "hg_sketch_stream_open", "hg_sketch_stream_push", "hg_sketch_stream_pop", "hg_sketch_stream_finish",
    "hg_sketch_stream_last_error", "hg_sketch_stream_close", "hg_sketch_stream_stats", "hg_device_numa_node", "hg_bind_thread_to_numa_node", "hg_dist_tile_order",
    "hg_sketch_stream_push_packed", "hg_pack2_size", "hg_pack2", "hg_unpack2_dev",
    "hg_sketch_stream_try_push", "hg_sketch_stream_max_pending",
    "hg_sketch_batch_dev_packed", "hg_pack2_batch_dev", "hg_pack2_dev",
    "hg_pack2s_size", "hg_pack2s", "hg_sketch_stream_push_packed_sparse",
    "hg_dist_ops_row_bytes", "hg_dist_ops_meta_bytes", "hg_dist_ops_padded_rows", "hg_dist_prep_ops_dev", "hg_dist_block_ops_dev",
    "hg_hv_packed_bytes_naive", "hg_hv_pack_naive", "hg_hv_unpack_naive", "hg_hv_payload_layout", "hg_hv_unpack_batch_dev",
    "hg_sketch_file_read_image", "hg_sketch_file_image", "hg_sketch_file_payload_offset",
    "hg_cluster_init_dev", "hg_cluster_add_hits_dev", "hg_cluster_finish_dev", "hg_cluster_dev", "hg_cluster",
    "hg_cluster_greedy_hits_dev", "hg_cluster_greedy_dev", "hg_cluster_greedy", "hg_ctx_cluster_greedy_rounds",
    "hg_cluster_setcover_hits_dev", "hg_cluster_setcover_dev", "hg_cluster_setcover", "hg_ctx_cluster_setcover_rounds",
    "hg_cluster_tree_hits_dev", "hg_cluster_tree_dev", "hg_cluster_tree", "hg_ctx_cluster_tree_rounds",
    "hg_cluster_average_matrix_dev", "hg_cluster_average_dev", "hg_cluster_average", "hg_ctx_cluster_average_rounds",
    "hg_cluster_complete_matrix_dev", "hg_cluster_complete_dev", "hg_cluster_complete", "hg_ctx_cluster_complete_rounds",
    "hg_cluster_stats_matrix_dev", "hg_cluster_stats_dev", "hg_cluster_stats",
    "hg_nj_matrix_dev", "hg_nj_dev", "hg_nj", "hg_nj_newick",
    "hg_ctx_set_ani_metric", "hg_ctx_ani_metric", "hg_multi_set_ani_metric",
    "hg_search_topk_dev", "hg_search_topk_block_dev", "hg_search_topk", "hg_search_topk_merge", "hg_search_topk_multi_dev",
    "hg_ani_pairs_dev", "hg_ani_pairs",
]
SEARCH_TOPK_MAX = 64  # HG_SEARCH_TOPK_MAX
CLUSTER_AVERAGE_MAX_N = 65536  # HG_CLUSTER_AVERAGE_MAX_N
CLUSTER_COMPLETE_MAX_N = 65536  # HG_CLUSTER_COMPLETE_MAX_N
STATS_NONE = 0xFFFFFFFF  # HG_STATS_NONE
NJ_MAX_N = 65536  # HG_NJ_MAX_N
NJ_FRAC_BITS = 15  # HG_NJ_FRAC_BITS: a branch length counts 2^-15 thousandths of an ANI percent
NJ_JOIN_DTYPE = np.dtype([("a", "<u4"), ("b", "<u4"), ("len_a", "<i8"), ("len_b", "<i8")])  # hg_nj_join, 24 bytes


class NodeStat(C.Structure):  # hg_node_stat
    _fields_ = [("within_sum", C.c_uint64), ("within_min", C.c_uint32), ("within_min_idx", C.c_uint32),
                ("outside_max", C.c_uint32), ("outside_max_idx", C.c_uint32)]


class ClusterStat(C.Structure):  # hg_cluster_stat
    _fields_ = [("within_sum", C.c_uint64), ("size", C.c_uint32), ("first", C.c_uint32), ("medoid", C.c_uint32),
                ("within_min", C.c_uint32), ("within_min_a", C.c_uint32), ("within_min_b", C.c_uint32),
                ("outside_max", C.c_uint32), ("outside_member", C.c_uint32), ("outside_idx", C.c_uint32), ("reserved", C.c_uint32)]


NODE_STAT_DTYPE = np.dtype([(name, np.uint64 if t is C.c_uint64 else np.uint32) for name, t in NodeStat._fields_])
CLUSTER_STAT_DTYPE = np.dtype([(name, np.uint64 if t is C.c_uint64 else np.uint32) for name, t in ClusterStat._fields_])


def source_stamp():
    """sha256 (first 16 hex digits) over the library's sources (csrc/* but the command-line tool hg_cli.cpp, which is not
    part of libhypergen_hip.so; include/hypergen.h), names and contents in sorted order.  tools/summarize_prof.py writes it into every profile summary and bench.py quotes a summary's counters only
    when the stamp equals that of the tree it runs from -- a kernel change without a re-profile then reports null
    instead of stale counters."""
    import hashlib
    h = hashlib.sha256()
    src = os.path.join(_HERE, "csrc")
    files = sorted(f for f in os.listdir(src) if (f.endswith((".hip", ".h", ".cpp")) or f == "Makefile") and f != "hg_cli.cpp")
    for f in [os.path.join(src, x) for x in files] + [os.path.join(_HERE, "..", "include", "hypergen.h")]:
        h.update(os.path.basename(f).encode() + b"\0")
        h.update(open(f, "rb").read())
    return h.hexdigest()[:16]


def cli_source_stamp():
    """source_stamp() extended by the command-line tool's source: what a measurement of the `hyper-gen` binary belongs to
    (bench.py's `cli` object and the profiles/rNN_cli_* files carry it)."""
    import hashlib
    h = hashlib.sha256(source_stamp().encode())
    h.update(open(os.path.join(_HERE, "csrc", "hg_cli.cpp"), "rb").read())
    return h.hexdigest()[:16]


def build(force=False):
    """Compile the library and CLI in-tree with hipcc for gfx950 (cross-compiles without a GPU)."""
    if force:
        subprocess.check_call(["make", "-s", "-C", os.path.join(_HERE, "csrc"), "clean"])
    subprocess.check_call(["make", "-s", "-j4", "-C", os.path.join(_HERE, "csrc"), "all"])


def _load(name, path, sig, exports=None, note=""):
    """The shared library `name` at `path` with restype / argtypes set from sig = {symbol: (restype, argtypes)}; sig must
    name exactly the symbols of `exports`, if given."""
    if not os.path.exists(path):
        raise ImportError("%s is not built: run `python -c 'import __graft_entry__ as g; g.build()'`%s" % (name, note))
    assert exports is None or sorted(sig) == sorted(exports)
    L = C.CDLL(path)
    for sym, (res, args) in sig.items():
        fn = getattr(L, sym)  # AttributeError here == the ABI lost a symbol
        fn.restype, fn.argtypes = res, args
    return L


_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    vp, sz = C.c_void_p, C.c_size_t
    u8p, u64p, i16p, i32p, u32p, f32p = (C.POINTER(t) for t in (
        C.c_uint8, C.c_uint64, C.c_int16, C.c_int32, C.c_uint32, C.c_float))
    sig = {
        "hg_status_str": (C.c_char_p, [C.c_int]),
        "hg_last_error": (C.c_char_p, [vp]),
        "hg_version": (C.c_char_p, []),
        "hg_ctx_create": (C.c_int, [C.c_int, C.POINTER(vp)]),
        "hg_ctx_destroy": (None, [vp]),
        "hg_ctx_set_stream": (C.c_int, [vp, vp]),
        "hg_ctx_reset_stream": (C.c_int, [vp]),
        "hg_ctx_sync": (C.c_int, [vp]),
        "hg_sketch_plan_describe": (C.c_int, [vp, vp, sz, C.c_uint32, C.c_uint64, C.POINTER(C.c_uint64), vp, sz]),
        "hg_logf_dev": (C.c_int, [vp, vp, C.c_uint32, sz, vp]),
        "hg_ani_from_dots_dev": (C.c_int, [vp, vp, vp, vp, sz, C.c_uint32, vp]),
        "hg_ctx_sketch_step_counts": (C.c_int, [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
        "hg_device_count": (C.c_int, []),
        "hg_dev_alloc": (C.c_int, [vp, sz, C.POINTER(vp)]),
        "hg_dev_free": (C.c_int, [vp, vp]),
        "hg_copy_h2d": (C.c_int, [vp, vp, vp, sz]),
        "hg_copy_d2h": (C.c_int, [vp, vp, vp, sz]),
        "hg_sketch_params_default": (None, [C.POINTER(SketchParams)]),
        "hg_kmer_hash_sample": (C.c_int, [vp, vp, sz, C.c_uint32, C.c_uint64, C.c_uint64, C.c_int,
                                          C.c_uint32, vp, sz, C.POINTER(sz)]),
        "hg_kmer_hash_sample_min_count": (C.c_int, [vp, vp, sz, C.c_uint32, C.c_uint64, C.c_uint64, C.c_int,
                                                    C.c_uint32, C.c_uint32, vp, sz, C.POINTER(sz)]),
        "hg_hv_encode": (C.c_int, [vp, vp, sz, C.c_uint32, C.c_uint32, vp, C.POINTER(C.c_int32)]),
        "hg_sketch_batch_dev": (C.c_int, [vp, vp, vp, vp, sz, C.POINTER(SketchParams), vp, vp, vp]),
        "hg_sketch_batch": (C.c_int, [vp, C.POINTER(vp), C.POINTER(sz), sz, C.POINTER(SketchParams),
                                      vp, vp, vp]),
        "hg_dist_full": (C.c_int, [vp, vp, vp, sz, vp, vp, sz, C.c_uint32, C.c_uint32, vp]),
        "hg_dist_full_dev": (C.c_int, [vp, vp, vp, sz, vp, vp, sz, C.c_uint32, C.c_uint32, vp]),
        "hg_ani_pairs_dev": (C.c_int, [vp, vp, vp, sz, vp, vp, sz, C.c_uint32, C.c_uint32, vp, sz, C.c_uint32, vp, vp]),
        "hg_ani_pairs": (C.c_int, [vp, vp, vp, sz, vp, vp, sz, C.c_uint32, C.c_uint32, vp, sz, C.c_uint32, vp, vp]),
        "hg_dist": (C.c_int, [vp, vp, vp, sz, vp, vp, sz, C.c_uint32, C.c_uint32, C.c_int, C.c_float,
                              vp, sz, C.POINTER(sz)]),
        "hg_dist_dev": (C.c_int, [vp, vp, vp, sz, vp, vp, sz, C.c_uint32, C.c_uint32, C.c_int,
                                  C.c_float, vp, sz, C.POINTER(sz)]),
        "hg_sort_ani_hits": (None, [vp, sz, sz, C.c_int]),
        "hg_hv_quant_bits": (C.c_uint32, [vp, C.c_uint32]),
        "hg_hv_pack": (C.c_int, [vp, C.c_uint32, C.c_uint32, vp]),
        "hg_hv_packed_bytes": (sz, [C.c_uint32, C.c_uint32]),
        "hg_hv_unpack": (C.c_int, [vp, C.c_uint32, C.c_uint32, vp]),
        "hg_sketch_file_write": (C.c_int, [C.c_char_p, C.POINTER(FileSketch), sz]),
        "hg_sketch_file_read": (C.c_int, [C.c_char_p, C.POINTER(vp)]),
        "hg_sketch_file_count": (sz, [vp]),
        "hg_sketch_file_get": (C.POINTER(FileSketch), [vp, sz]),
        "hg_sketch_file_free": (None, [vp]),
        "hg_read_merge_seq": (C.c_int, [C.c_char_p, C.POINTER(vp), C.POINTER(sz)]),
        "hg_read_merge_seq_into": (C.c_int, [C.c_char_p, C.POINTER(vp), C.POINTER(sz), C.POINTER(sz)]),
        "hg_read_fastx_into": (C.c_int, [C.c_char_p, C.c_uint32, C.POINTER(vp), C.POINTER(sz), C.POINTER(sz)]),
        "hg_ctx_set_debug": (C.c_int, [vp, C.c_char_p, C.c_char_p]),
        "hg_free": (None, [vp]),
        "hg_read_fastx_pinned": (C.c_int, [C.c_char_p, C.c_uint32, C.POINTER(vp), C.POINTER(sz), C.POINTER(sz)]),
        "hg_pinned_free": (None, [vp]),
        "hg_device_numa_node": (C.c_int, [C.c_int]),
        "hg_bind_thread_to_numa_node": (C.c_int, [C.c_int, C.c_uint]),
        "hg_dist_tile_order": (C.c_int, [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.c_uint64, C.c_uint64,
                                         C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]),
        "hg_sketch_stream_open": (C.c_int, [C.POINTER(C.c_int), C.c_int, C.POINTER(SketchParams), C.POINTER(vp)]),
        "hg_sketch_stream_push": (C.c_int, [vp, vp, sz, C.c_uint64]),
        "hg_sketch_stream_pop": (C.c_int, [vp, C.POINTER(C.c_uint64), vp, C.POINTER(C.c_int32), C.POINTER(C.c_uint32),
                                           C.POINTER(C.c_int)]),
        "hg_sketch_stream_push_packed": (C.c_int, [vp, vp, sz, C.c_uint64]),
        "hg_sketch_stream_try_push": (C.c_int, [vp, vp, sz, C.c_uint64, C.c_int]),
        "hg_sketch_stream_max_pending": (sz, [vp]),
        "hg_pack2_size": (sz, [sz]),
        "hg_pack2": (C.c_int, [vp, sz, C.c_uint32, vp]),
        "hg_unpack2_dev": (C.c_int, [vp, vp, sz, vp]),
        "hg_sketch_batch_dev_packed": (C.c_int, [vp, vp, vp, vp, sz, C.POINTER(SketchParams), vp, vp, vp]),
        "hg_pack2_batch_dev": (C.c_int, [vp, vp, vp, vp, sz, C.c_uint32, vp, vp]),
        "hg_pack2_dev": (C.c_int, [vp, vp, sz, C.c_uint32, vp]),
        "hg_dist_ops_row_bytes": (sz, [C.c_uint32]),
        "hg_dist_ops_meta_bytes": (sz, []),
        "hg_dist_ops_padded_rows": (sz, [sz]),
        "hg_dist_prep_ops_dev": (C.c_int, [vp, vp, sz, C.c_uint32, vp, vp, vp]),
        "hg_dist_block_ops_dev": (C.c_int, [vp, vp, vp, vp, sz, sz, vp, vp, sz, vp, vp, sz, sz, C.c_uint32, C.c_uint32, C.c_int,
                                            C.c_float, vp, sz, C.POINTER(sz)]),
        "hg_pack2s_size": (sz, [sz, sz]),
        "hg_pack2s": (C.c_int, [vp, sz, C.c_uint32, vp, sz, C.POINTER(sz)]),
        "hg_sketch_stream_push_packed_sparse": (C.c_int, [vp, vp, sz, sz, C.c_uint64]),
        "hg_sketch_stream_finish": (C.c_int, [vp]),
        "hg_sketch_stream_last_error": (C.c_char_p, [vp]),
        "hg_sketch_stream_close": (None, [vp]),
        "hg_sketch_stream_stats": (C.c_int, [vp, C.c_int, C.POINTER(C.c_double)]),
        "hg_ctx_last_dist_path": (C.c_int, [vp]),
        "hg_ctx_set_ani_metric": (C.c_int, [vp, C.c_int]),
        "hg_ctx_ani_metric": (C.c_int, [vp]),
        "hg_multi_set_ani_metric": (C.c_int, [vp, C.c_int]),
        "hg_ctx_last_hamming_path": (C.c_int, [vp]),
        "hg_sort_ani_hits_dev": (C.c_int, [vp, vp, sz, sz]),
        "hg_sort_ani_hits_staged": (C.c_int, [vp, vp, sz, sz]),
        "hg_topk_per_query_dev": (C.c_int, [vp, vp, sz, sz, C.c_uint32, vp, vp]),
        "hg_dist_block_dev": (C.c_int, [vp, vp, vp, sz, sz, vp, vp, sz, sz, C.c_uint32, C.c_uint32, C.c_int,
                                        C.c_float, vp, sz, C.POINTER(sz)]),
        "hg_hamming_search_block_dev": (C.c_int, [vp, vp, sz, sz, vp, sz, sz, C.c_uint32, C.c_uint32, vp, sz,
                                                  C.POINTER(sz)]),
        "hg_multi_create": (C.c_int, [C.POINTER(C.c_int), C.c_int, C.POINTER(vp)]),
        "hg_multi_destroy": (None, [vp]),
        "hg_multi_size": (C.c_int, [vp]),
        "hg_multi_ctx": (vp, [vp, C.c_int]),
        "hg_multi_last_error": (C.c_char_p, [vp]),
        "hg_multi_peer_report": (C.c_char_p, [vp]),
        "hg_multi_gather_report": (C.c_char_p, [vp]),
        "hg_multi_set_gather": (C.c_int, [vp, C.c_int]),
        "hg_multi_gather_mode": (C.c_int, [vp]),
        "hg_shard_range": (None, [sz, C.c_int, C.c_int, C.POINTER(sz), C.POINTER(sz)]),
        "hg_sketch_batch_multi": (C.c_int, [vp, C.POINTER(vp), C.POINTER(sz), sz, C.POINTER(SketchParams),
                                            vp, vp, vp]),
        "hg_dist_multi": (C.c_int, [vp, vp, vp, sz, vp, vp, sz, C.c_uint32, C.c_uint32, C.c_int, C.c_float,
                                    vp, sz, C.POINTER(sz)]),
        "hg_dist_multi_dev": (C.c_int, [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(sz), C.POINTER(vp),
                                        C.POINTER(vp), C.POINTER(sz), C.c_uint32, C.c_uint32, C.c_int,
                                        C.c_float, vp, sz, C.POINTER(sz)]),
        "hg_hamming_search_multi": (C.c_int, [vp, vp, sz, vp, sz, C.c_uint32, C.c_uint32, vp, sz, C.POINTER(sz)]),
        "hg_hv_binarize_dev": (C.c_int, [vp, vp, sz, C.c_uint32, vp]),
        "hg_hamming_full_dev": (C.c_int, [vp, vp, sz, vp, sz, C.c_uint32, vp]),
        "hg_hamming_search_dev": (C.c_int, [vp, vp, sz, vp, sz, C.c_uint32, C.c_uint32, vp, sz, C.POINTER(sz)]),
        "hg_ctx_enable_timing": (C.c_int, [vp, C.c_int]),
        "hg_ctx_last_kernel": (C.c_char_p, [vp, C.c_int]),
        "hg_ctx_timings": (C.c_int, [vp, C.POINTER(C.c_float), C.POINTER(C.c_uint32)]),
        "hg_synth_genomes_dev": (C.c_int, [vp, C.c_uint64, sz, C.c_uint64, C.c_uint32, C.c_uint32,
                                           C.c_uint64, vp]),
        "hg_hv_packed_bytes_naive": (sz, [C.c_uint32, C.c_uint32]),
        "hg_hv_pack_naive": (C.c_int, [vp, C.c_uint32, C.c_uint32, vp]),
        "hg_hv_unpack_naive": (C.c_int, [vp, C.c_uint32, C.c_uint32, vp]),
        "hg_hv_payload_layout": (C.c_int, [C.c_uint32, C.c_uint32, sz]),
        "hg_hv_unpack_batch_dev": (C.c_int, [vp, vp, sz, vp, vp, vp, sz, C.c_uint32, vp]),
        "hg_sketch_file_read_image": (C.c_int, [C.c_char_p, C.POINTER(vp)]),
        "hg_sketch_file_image": (vp, [vp, C.POINTER(sz)]),
        "hg_sketch_file_payload_offset": (C.c_uint64, [vp, sz]),
        "hg_cluster_init_dev": (C.c_int, [vp, vp, sz]),
        "hg_cluster_add_hits_dev": (C.c_int, [vp, vp, sz, vp, sz, C.c_float]),
        "hg_cluster_finish_dev": (C.c_int, [vp, vp, sz, vp, C.POINTER(sz)]),
        "hg_cluster_dev": (C.c_int, [vp, vp, vp, sz, C.c_uint32, C.c_uint32, C.c_float, vp, vp, C.POINTER(sz)]),
        "hg_cluster": (C.c_int, [vp, vp, vp, sz, C.c_uint32, C.c_uint32, C.c_float, vp, vp, C.POINTER(sz)]),
        "hg_cluster_greedy_hits_dev": (C.c_int, [vp, sz, vp, sz, C.c_float, vp, vp, vp, C.POINTER(sz)]),
        "hg_cluster_greedy_dev": (C.c_int, [vp, vp, vp, sz, C.c_uint32, C.c_uint32, C.c_float, vp, vp, vp, C.POINTER(sz)]),
        "hg_cluster_greedy": (C.c_int, [vp, vp, vp, sz, C.c_uint32, C.c_uint32, C.c_float, vp, vp, vp, C.POINTER(sz)]),
        "hg_ctx_cluster_greedy_rounds": (C.c_uint64, [vp]),
        "hg_cluster_setcover_hits_dev": (C.c_int, [vp, sz, vp, sz, C.c_float, vp, vp, vp, C.POINTER(sz)]),
        "hg_cluster_setcover_dev": (C.c_int, [vp, vp, vp, sz, C.c_uint32, C.c_uint32, C.c_float, vp, vp, vp, C.POINTER(sz)]),
        "hg_cluster_setcover": (C.c_int, [vp, vp, vp, sz, C.c_uint32, C.c_uint32, C.c_float, vp, vp, vp, C.POINTER(sz)]),
        "hg_ctx_cluster_setcover_rounds": (C.c_uint64, [vp]),
        "hg_cluster_tree_hits_dev": (C.c_int, [vp, sz, vp, sz, C.c_float, vp, sz, C.POINTER(sz), vp, vp, C.POINTER(sz)]),
        "hg_cluster_tree_dev": (C.c_int, [vp, vp, vp, sz, C.c_uint32, C.c_uint32, C.c_float, vp, sz, C.POINTER(sz), vp, vp, C.POINTER(sz)]),
        "hg_cluster_tree": (C.c_int, [vp, vp, vp, sz, C.c_uint32, C.c_uint32, C.c_float, vp, sz, C.POINTER(sz), vp, vp, C.POINTER(sz)]),
        "hg_ctx_cluster_tree_rounds": (C.c_uint64, [vp]),
        "hg_cluster_average_matrix_dev": (C.c_int, [vp, vp, sz, C.c_float, vp, vp, vp, vp, vp, C.POINTER(sz)]),
        "hg_cluster_average_dev": (C.c_int, [vp, vp, vp, sz, C.c_uint32, C.c_uint32, C.c_float, vp, vp, vp, vp, vp, C.POINTER(sz)]),
        "hg_cluster_average": (C.c_int, [vp, vp, vp, sz, C.c_uint32, C.c_uint32, C.c_float, vp, vp, vp, vp, vp, C.POINTER(sz)]),
        "hg_ctx_cluster_average_rounds": (C.c_uint64, [vp]),
        "hg_cluster_complete_matrix_dev": (C.c_int, [vp, vp, sz, C.c_float, vp, vp, vp, vp, vp, C.POINTER(sz)]),
        "hg_cluster_complete_dev": (C.c_int, [vp, vp, vp, sz, C.c_uint32, C.c_uint32, C.c_float, vp, vp, vp, vp, vp, C.POINTER(sz)]),
        "hg_cluster_complete": (C.c_int, [vp, vp, vp, sz, C.c_uint32, C.c_uint32, C.c_float, vp, vp, vp, vp, vp, C.POINTER(sz)]),
        "hg_ctx_cluster_complete_rounds": (C.c_uint64, [vp]),
        "hg_cluster_stats_matrix_dev": (C.c_int, [vp, vp, sz, vp, sz, vp, vp]),
        "hg_cluster_stats_dev": (C.c_int, [vp, vp, vp, sz, C.c_uint32, C.c_uint32, vp, sz, vp, vp]),
        "hg_cluster_stats": (C.c_int, [vp, vp, vp, sz, C.c_uint32, C.c_uint32, vp, sz, vp, vp]),
        "hg_nj_matrix_dev": (C.c_int, [vp, vp, sz, vp, C.POINTER(sz)]),
        "hg_nj_dev": (C.c_int, [vp, vp, vp, sz, C.c_uint32, C.c_uint32, vp, C.POINTER(sz)]),
        "hg_nj": (C.c_int, [vp, vp, vp, sz, C.c_uint32, C.c_uint32, vp, C.POINTER(sz)]),
        "hg_nj_newick": (C.c_int, [vp, sz, C.POINTER(C.c_char_p), C.POINTER(vp), C.POINTER(sz)]),
        "hg_search_topk_dev": (C.c_int, [vp, vp, vp, sz, vp, vp, sz, C.c_uint32, C.c_uint32, C.c_float, C.c_uint32, vp, vp]),
        "hg_search_topk_block_dev": (C.c_int, [vp, vp, vp, sz, sz, vp, vp, sz, sz, C.c_uint32, C.c_uint32, C.c_float, C.c_uint32,
                                               vp, vp]),
        "hg_search_topk": (C.c_int, [vp, vp, vp, sz, vp, vp, sz, C.c_uint32, C.c_uint32, C.c_float, C.c_uint32, vp, vp]),
        "hg_search_topk_merge": (C.c_int, [C.POINTER(vp), C.POINTER(vp), sz, sz, C.c_uint32, vp, vp]),
        "hg_search_topk_multi_dev": (C.c_int, [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(sz), C.POINTER(vp), C.POINTER(vp), sz,
                                               C.c_uint32, C.c_uint32, C.c_float, C.c_uint32, vp, vp]),
    }
    _lib = _load("libhypergen_hip.so", LIB_PATH, sig, note=" (there is no CPU fallback)")
    return _lib


def _ptr(a):
    return C.c_void_p(a.ctypes.data) if isinstance(a, np.ndarray) else C.c_void_p(int(a))


def _u8(seq):
    """bytes or an array as a contiguous uint8 array"""
    return np.ascontiguousarray(seq if isinstance(seq, np.ndarray) else np.frombuffer(bytes(seq), np.uint8), dtype=np.uint8)


def _sketch_batch_host(ck, fn, handle, seqs, p):
    """one of the host-memory batch sketchers on a list of sequences: (hv, norm2, nhash)"""
    arrs = [_u8(s) for s in seqs]
    n = len(arrs)
    ptrs = (C.c_void_p * max(n, 1))(*[a.ctypes.data if a.size else None for a in arrs])
    lens = (C.c_size_t * max(n, 1))(*[a.size for a in arrs])
    hv = np.zeros((n, p.hv_d), np.int16)
    n2 = np.zeros(n, np.int32)
    nh = np.zeros(n, np.uint32)
    ck(fn(handle, ptrs, lens, n, C.byref(p), _ptr(hv), _ptr(n2), _ptr(nh)))
    return hv, n2, nh


def _sized_then_called(call, seq_cap, rec_cap):
    """a splitter call(seq_cap, rec_cap) -> (status, n_recs, seq_bytes, recs, seq); without capacities a first call sizes
    the outputs: rec_cap = n_recs and seq_cap = seq_bytes + 32"""
    if seq_cap is None or rec_cap is None:
        st, n_recs, seq_bytes, _, _ = call(0, 0)
        if st != ERR_CAPACITY:
            return st, n_recs, seq_bytes, np.zeros(0, REC_DTYPE), np.zeros(0, np.uint8)
        seq_cap, rec_cap = seq_bytes + 32, n_recs
    return call(seq_cap, rec_cap)


# ---- libhypergen_aa.so (include/hypergen_aa.h): amino-acid k-mer sketches; the contexts are this module's ----
AA_LIB_PATH = os.path.join(_HERE, "libhypergen_aa.so")
AA_EXPORTS = [
    "hg_aa_hash_sample", "hg_aa_sketch_batch_dev", "hg_aa_sketch_batch", "hg_aa_read_fasta", "hg_aa_kernel_name",
    "hg_aa_tile_starts", "hg_aa_item_starts",
]


@functools.lru_cache(None)
def lib_aa():
    """The companion library, loaded behind lib() (it links libhypergen_hip.so; the loader finds the copy already in the process)."""
    lib()
    vp, sz = C.c_void_p, C.c_size_t
    sig = {
        "hg_aa_hash_sample": (C.c_int, [vp, vp, sz, C.c_uint32, C.c_uint64, C.c_uint64, vp, sz, C.POINTER(sz)]),
        "hg_aa_sketch_batch_dev": (C.c_int, [vp, vp, vp, vp, sz, C.POINTER(SketchParams), vp, vp, vp]),
        "hg_aa_sketch_batch": (C.c_int, [vp, C.POINTER(vp), C.POINTER(sz), sz, C.POINTER(SketchParams), vp, vp, vp]),
        "hg_aa_read_fasta": (C.c_int, [C.c_char_p, C.POINTER(vp), C.POINTER(sz), C.POINTER(sz)]),
        "hg_aa_kernel_name": (C.c_char_p, [C.c_uint32]),
        "hg_aa_tile_starts": (C.c_uint32, []),
        "hg_aa_item_starts": (C.c_uint32, [C.c_uint32]),
    }
    return _load("libhypergen_aa.so", AA_LIB_PATH, sig, AA_EXPORTS)


def _read_file(read, free, what, path):
    """read(path, byref(buffer), byref(capacity), byref(n)) -> status; the n bytes it left in the buffer, which free() releases"""
    buf, cap, n = C.c_void_p(), C.c_size_t(0), C.c_size_t(0)
    st = read(os.fsencode(path), C.byref(buf), C.byref(cap), C.byref(n))
    try:
        if st != OK:
            raise HgError(st, "%s: %s" % (what, path))
        return C.string_at(buf, n.value)
    finally:
        free(buf)


def aa_read_fasta(path):
    """hg_aa_read_fasta: a protein FASTA file (plain or gzip) as one proteome, a uint8 array -- the records' sequence bytes with
    line ends, blanks, tabs and CRs dropped and one '*' at every record start.  Needs no GPU."""
    return np.frombuffer(_read_file(lib_aa().hg_aa_read_fasta, lib().hg_free, "hg_aa_read_fasta", path), np.uint8).copy()


def aa_kernel_name(ksize):
    """hg_aa_kernel_name: what Context.last_kernel("kmer") reports after an amino-acid call with this ksize"""
    return lib_aa().hg_aa_kernel_name(ksize).decode()


def aa_tile_starts():
    return int(lib_aa().hg_aa_tile_starts())


def aa_item_starts(ksize):
    return int(lib_aa().hg_aa_item_starts(ksize))


# ---- libhypergen_tx.so (include/hypergen_tx.h): six-frame translated protein sketches from DNA ----
TX_LIB_PATH = os.path.join(_HERE, "libhypergen_tx.so")
TX_EXPORTS = [
    "hg_tx_hash_sample", "hg_tx_sketch_batch_dev", "hg_tx_sketch_batch", "hg_tx_translate_frame", "hg_tx_kernel_name",
    "hg_tx_tile_starts", "hg_tx_item_starts", "hg_tx_plan_describe", "hg_tx_plan_regrows",
]


@functools.lru_cache(None)
def lib_tx():
    """The second companion library, loaded behind lib() like lib_aa()."""
    lib()
    vp, sz = C.c_void_p, C.c_size_t
    sig = {
        "hg_tx_hash_sample": (C.c_int, [vp, vp, sz, C.c_uint32, C.c_uint64, C.c_uint64, vp, sz, C.POINTER(sz)]),
        "hg_tx_sketch_batch_dev": (C.c_int, [vp, vp, vp, vp, sz, C.POINTER(SketchParams), vp, vp, vp]),
        "hg_tx_sketch_batch": (C.c_int, [vp, C.POINTER(vp), C.POINTER(sz), sz, C.POINTER(SketchParams), vp, vp, vp]),
        "hg_tx_translate_frame": (C.c_int, [vp, sz, C.c_uint32, vp, sz, C.POINTER(sz)]),
        "hg_tx_kernel_name": (C.c_char_p, [C.c_uint32]),
        "hg_tx_tile_starts": (C.c_uint32, []),
        "hg_tx_item_starts": (C.c_uint32, [C.c_uint32]),
        "hg_tx_plan_describe": (C.c_int, [vp, vp, sz, C.c_uint32, C.c_uint64, vp]),
        "hg_tx_plan_regrows": (C.c_uint64, [vp]),
    }
    return _load("libhypergen_tx.so", TX_LIB_PATH, sig, TX_EXPORTS)


def tx_translate_frame(seq, frame):
    """hg_tx_translate_frame: reading frame 0..5 of a nucleotide sequence as bytes, stops '*', codons with a non-base 'X'.
    Needs no GPU."""
    a = _u8(seq)
    out = np.zeros(a.size // 3 + 1, np.uint8)
    n = C.c_size_t(0)
    st = lib_tx().hg_tx_translate_frame(_ptr(a) if a.size else None, a.size, frame, _ptr(out), out.size, C.byref(n))
    if st != OK:
        raise HgError(st, "hg_tx_translate_frame")
    return out[: n.value].tobytes()


def tx_plan_describe(lens, ksize, scaled, offsets=None):
    """hg_tx_plan_describe: dict of the translated plan's figures for genomes of these lengths (offsets default to a 64-byte grid)"""
    ln = np.ascontiguousarray(lens, np.uint64)
    if offsets is None:
        offsets = np.concatenate(([0], np.cumsum((ln + np.uint64(32 + 63)) // np.uint64(64) * np.uint64(64))[:-1])) if ln.size else []
    off = np.ascontiguousarray(offsets, np.uint64)
    counts = np.zeros(6, np.uint64)
    st = lib_tx().hg_tx_plan_describe(_ptr(off), _ptr(ln), ln.size, ksize, C.c_uint64(scaled), _ptr(counts))
    if st != OK:
        raise HgError(st, "hg_tx_plan_describe")
    return dict(zip(("items", "slots", "max_cap", "min_cap", "max_expect", "item_starts"), (int(x) for x in counts)))


def tx_kernel_name(ksize):
    """hg_tx_kernel_name: what Context.last_kernel("kmer") reports after a translated call with this ksize"""
    return lib_tx().hg_tx_kernel_name(ksize).decode()


def tx_tile_starts():
    return int(lib_tx().hg_tx_tile_starts())


def tx_item_starts(ksize):
    return int(lib_tx().hg_tx_item_starts(ksize))


# ---- libhypergen_rec.so (include/hypergen_rec.h): one multi-FASTA text split into its records on the device ----
REC_LIB_PATH = os.path.join(_HERE, "libhypergen_rec.so")
REC_EXPORTS = [
    "hg_rec_count_dev", "hg_rec_split_dev", "hg_rec_split", "hg_rec_split_host", "hg_rec_read_text", "hg_rec_sketch_text_dev",
    "hg_rec_block_bytes", "hg_rec_kernel_names", "hg_rec_launch_counts",
]
REC_DTYPE = np.dtype([("hdr_off", np.uint64), ("hdr_len", np.uint32), ("id_len", np.uint32), ("seq_off", np.uint64),
                      ("seq_len", np.uint64)])  # hg_rec_entry
REC_ROWS_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p)


@functools.lru_cache(None)
def lib_rec():
    """The third companion library, loaded behind lib() like lib_aa()."""
    lib()
    vp, sz = C.c_void_p, C.c_size_t
    sig = {
        "hg_rec_count_dev": (C.c_int, [vp, vp, sz, C.POINTER(sz), C.POINTER(sz)]),
        "hg_rec_split_dev": (C.c_int, [vp, vp, sz, vp, sz, vp, sz, C.POINTER(sz), C.POINTER(sz)]),
        "hg_rec_split": (C.c_int, [vp, vp, sz, vp, sz, vp, sz, C.POINTER(sz), C.POINTER(sz)]),
        "hg_rec_split_host": (C.c_int, [vp, sz, vp, sz, vp, sz, C.POINTER(sz), C.POINTER(sz)]),
        "hg_rec_read_text": (C.c_int, [C.c_char_p, C.POINTER(vp), C.POINTER(sz), C.POINTER(sz)]),
        "hg_rec_sketch_text_dev": (C.c_int, [vp, vp, sz, C.POINTER(SketchParams), C.c_uint64, REC_ROWS_FN, vp, C.POINTER(sz), C.POINTER(sz)]),
        "hg_rec_block_bytes": (C.c_uint32, []),
        "hg_rec_kernel_names": (C.c_char_p, []),
        "hg_rec_launch_counts": (C.c_uint32, [vp, C.c_uint32]),
    }
    return _load("libhypergen_rec.so", REC_LIB_PATH, sig, REC_EXPORTS)


def rec_block_bytes():
    """hg_rec_block_bytes: bytes of text per workgroup of the per-block kernels"""
    return int(lib_rec().hg_rec_block_bytes())


def rec_kernel_names():
    """hg_rec_kernel_names: the library's kernels as rocprofv3 spells them, in launch order"""
    return lib_rec().hg_rec_kernel_names().decode().split("\n")


def rec_launch_counts():
    """hg_rec_launch_counts: {kernel name: launches of this process so far}"""
    names = rec_kernel_names()
    counts = np.zeros(len(names), np.uint64)
    assert lib_rec().hg_rec_launch_counts(_ptr(counts), counts.size) == len(names)
    return dict(zip(names, (int(x) for x in counts)))


def _rec_host_call(fn, text, seq_cap, rec_cap, fill):
    """one of the host-memory splitters on `text`: (status, n_recs, seq_bytes, record table of rec_cap entries, buffer of seq_cap
    bytes); both outputs are filled with `fill` before the call"""
    a = np.frombuffer(bytes(text), np.uint8)
    seq = np.full(seq_cap, fill, np.uint8)
    recs = np.frombuffer(np.full(rec_cap * REC_DTYPE.itemsize, fill, np.uint8).tobytes(), REC_DTYPE).copy()
    n_recs, seq_bytes = C.c_size_t(0), C.c_size_t(0)
    st = fn(_ptr(a) if a.size else None, a.size, _ptr(seq) if seq_cap else None, seq_cap, _ptr(recs) if rec_cap else None, rec_cap,
            C.byref(n_recs), C.byref(seq_bytes))
    return st, int(n_recs.value), int(seq_bytes.value), recs, seq


def rec_split_host(text, seq_cap=None, rec_cap=None, fill=0xEE):
    """hg_rec_split_host (one host thread, needs no GPU).  Without capacities: a first call sizes the outputs, rec_cap = n_recs and
    seq_cap = seq_bytes + 32.  Returns (status, n_recs, seq_bytes, recs, seq)."""
    return _sized_then_called(lambda sc, rc: _rec_host_call(lib_rec().hg_rec_split_host, text, sc, rc, fill), seq_cap, rec_cap)


def rec_read_text(path):
    """hg_rec_read_text: the bytes of a file, gzip inflated, read into page-locked memory (needs the HIP runtime)"""
    return _read_file(lib_rec().hg_rec_read_text, lib().hg_pinned_free, "hg_rec_read_text", path)


# ---- libhypergen_frag.so (include/hypergen_frag.h): fragment-wise ANI and aligned fraction ----
FRAG_LIB_PATH = os.path.join(_HERE, "libhypergen_frag.so")
FRAG_EXPORTS = [
    "hg_frag_plan", "hg_frag_sketch_seq_dev", "hg_frag_ani_matrix_dev", "hg_frag_ani_dev", "hg_frag_ani", "hg_frag_row_chunk",
    "hg_frag_col_tile", "hg_frag_wave", "hg_frag_fold_threads", "hg_frag_kernel_names", "hg_frag_launch_counts",
]
FRAG_PAIR_DTYPE = np.dtype([("sum", np.uint64), ("matched", np.uint32), ("total", np.uint32)])  # hg_frag_pair
FRAG_BEST_DTYPE = np.dtype([("m", np.uint32), ("row", np.uint32)])  # hg_frag_best
FRAG_NONE = 0xFFFFFFFF
FRAG_ROWS_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p)


@functools.lru_cache(None)
def lib_frag():
    """The fourth companion library, loaded behind lib() like lib_aa()."""
    lib()
    vp, sz, u64 = C.c_void_p, C.c_size_t, C.c_uint64
    sig = {
        "hg_frag_plan": (C.c_int, [u64, u64, u64, vp, vp, sz, C.POINTER(sz)]),
        "hg_frag_sketch_seq_dev": (C.c_int, [vp, vp, u64, C.POINTER(SketchParams), u64, u64, FRAG_ROWS_FN, vp, C.POINTER(sz)]),
        "hg_frag_ani_matrix_dev": (C.c_int, [vp, vp, sz, sz, vp, sz, vp, sz, C.c_float, vp, vp]),
        "hg_frag_ani_dev": (C.c_int, [vp, vp, vp, sz, vp, vp, sz, C.c_uint32, C.c_uint32, vp, sz, vp, sz, C.c_float, sz, vp, vp]),
        "hg_frag_ani": (C.c_int, [vp, vp, vp, sz, vp, vp, sz, C.c_uint32, C.c_uint32, vp, sz, vp, sz, C.c_float, vp, vp]),
        "hg_frag_row_chunk": (C.c_uint32, []),
        "hg_frag_col_tile": (C.c_uint32, []),
        "hg_frag_wave": (C.c_uint32, []),
        "hg_frag_fold_threads": (C.c_uint32, []),
        "hg_frag_kernel_names": (C.c_char_p, []),
        "hg_frag_launch_counts": (C.c_uint32, [vp, C.c_uint32]),
    }
    return _load("libhypergen_frag.so", FRAG_LIB_PATH, sig, FRAG_EXPORTS)


def frag_plan(length, window, step, cap=None):
    """hg_frag_plan (needs no GPU): (status, n, starts, lens); without a capacity a first call sizes the arrays"""
    n = C.c_size_t(0)
    if cap is None:
        st = lib_frag().hg_frag_plan(length, window, step, None, None, 0, C.byref(n))
        if st != ERR_CAPACITY:
            return st, int(n.value), np.zeros(0, np.uint64), np.zeros(0, np.uint64)
        cap = int(n.value)
    starts, lens = np.zeros(cap, np.uint64), np.zeros(cap, np.uint64)
    st = lib_frag().hg_frag_plan(length, window, step, _ptr(starts) if cap else None, _ptr(lens) if cap else None, cap, C.byref(n))
    return st, int(n.value), starts, lens


def frag_geometry():
    """dict of hg_frag_row_chunk, hg_frag_col_tile, hg_frag_wave and hg_frag_fold_threads"""
    L = lib_frag()
    return {"row_chunk": int(L.hg_frag_row_chunk()), "col_tile": int(L.hg_frag_col_tile()), "wave": int(L.hg_frag_wave()),
            "fold_threads": int(L.hg_frag_fold_threads())}


def frag_kernel_names():
    """hg_frag_kernel_names: the library's kernels as rocprofv3 spells them, in launch order"""
    return lib_frag().hg_frag_kernel_names().decode().split("\n")


def frag_launch_counts():
    """hg_frag_launch_counts: {kernel name: launches of this process so far}"""
    names = frag_kernel_names()
    counts = np.zeros(len(names), np.uint64)
    assert lib_frag().hg_frag_launch_counts(_ptr(counts), counts.size) == len(names)
    return dict(zip(names, (int(x) for x in counts)))


def _frag_offsets(first):
    """genome offsets as the uint32 array the library reads, and the number of genomes"""
    a = np.ascontiguousarray(first, np.uint32)
    return a, max(a.size - 1, 0)


# ---- libhypergen_hist.so (include/hypergen_hist.h): the histogram of the ANI values of a whole comparison ----
HIST_LIB_PATH = os.path.join(_HERE, "libhypergen_hist.so")
HIST_EXPORTS = [
    "hg_hist_bins", "hg_hist_add_matrix_dev", "hg_hist_dev", "hg_hist", "hg_hist_lds_bins", "hg_hist_tile_rows", "hg_hist_tile_cols",
    "hg_hist_threads", "hg_hist_kernel_names", "hg_hist_launch_counts",
]
HIST_ALL, HIST_UPPER, HIST_OFFDIAG = 0, 1, 2  # HG_HIST_*: every (i, j); i < j; i != j
HIST_MILLI_MAX = 100000  # HG_HIST_MILLI_MAX


@functools.lru_cache(None)
def lib_hist():
    """The fifth companion library, loaded behind lib() like lib_aa()."""
    lib()
    vp, sz, u32 = C.c_void_p, C.c_size_t, C.c_uint32
    sig = {
        "hg_hist_bins": (u32, [u32]),
        "hg_hist_add_matrix_dev": (C.c_int, [vp, vp, sz, sz, sz, sz, sz, u32, u32, vp]),
        "hg_hist_dev": (C.c_int, [vp, vp, vp, sz, vp, vp, sz, u32, u32, u32, u32, sz, vp]),
        "hg_hist": (C.c_int, [vp, vp, vp, sz, vp, vp, sz, u32, u32, u32, u32, vp]),
        "hg_hist_lds_bins": (u32, []),
        "hg_hist_tile_rows": (u32, []),
        "hg_hist_tile_cols": (u32, []),
        "hg_hist_threads": (u32, []),
        "hg_hist_kernel_names": (C.c_char_p, []),
        "hg_hist_launch_counts": (u32, [vp, u32]),
    }
    return _load("libhypergen_hist.so", HIST_LIB_PATH, sig, HIST_EXPORTS)


def hist_bins(bin_milli):
    """hg_hist_bins (needs no GPU): the bins of a width in thousandths, 0 for a width outside 1..100 000"""
    return int(lib_hist().hg_hist_bins(bin_milli))


def hist_geometry():
    """dict of hg_hist_lds_bins, hg_hist_tile_rows, hg_hist_tile_cols and hg_hist_threads"""
    L = lib_hist()
    return {"lds_bins": int(L.hg_hist_lds_bins()), "tile_rows": int(L.hg_hist_tile_rows()), "tile_cols": int(L.hg_hist_tile_cols()),
            "threads": int(L.hg_hist_threads())}


def hist_kernel_names():
    """hg_hist_kernel_names: the library's kernels as rocprofv3 spells them"""
    return lib_hist().hg_hist_kernel_names().decode().split("\n")


def hist_launch_counts():
    """hg_hist_launch_counts: {kernel name: launches of this process so far}"""
    names = hist_kernel_names()
    counts = np.zeros(len(names), np.uint64)
    assert lib_hist().hg_hist_launch_counts(_ptr(counts), counts.size) == len(names)
    return dict(zip(names, (int(x) for x in counts)))


# ---- libhypergen_tri.so (include/hypergen_tri.h): the ANI matrix of all pairs of one set as fixed-width text ----
TRI_LIB_PATH = os.path.join(_HERE, "libhypergen_tri.so")
TRI_EXPORTS = [
    "hg_tri_text_bytes", "hg_tri_field_offset", "hg_tri_format_dev", "hg_tri_dev", "hg_tri_stream_dev", "hg_tri", "hg_tri_tile_rows",
    "hg_tri_tile_cols", "hg_tri_threads", "hg_tri_kernel_names", "hg_tri_launch_counts",
]
TRI_LOWER, TRI_FULL = 0, 1  # HG_TRI_*: the fields j < i of row i; all of them
TRI_FIELD_BYTES = 8  # HG_TRI_FIELD_BYTES
TRI_SINK = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t)  # hg_tri_sink


@functools.lru_cache(None)
def lib_tri():
    """The sixth companion library, loaded behind lib() like lib_aa()."""
    lib()
    vp, sz, u32, u64 = C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint64
    sig = {
        "hg_tri_text_bytes": (u64, [u32, u64, u64, u64]),
        "hg_tri_field_offset": (u64, [u32, u64, u64, u64, u64]),
        "hg_tri_format_dev": (C.c_int, [vp, vp, sz, sz, sz, sz, u32, vp]),
        "hg_tri_dev": (C.c_int, [vp, vp, vp, sz, u32, u32, u32, sz, vp]),
        "hg_tri_stream_dev": (C.c_int, [vp, vp, vp, sz, u32, u32, u32, sz, TRI_SINK, vp]),
        "hg_tri": (C.c_int, [vp, vp, vp, sz, u32, u32, u32, vp]),
        "hg_tri_tile_rows": (u32, []),
        "hg_tri_tile_cols": (u32, []),
        "hg_tri_threads": (u32, []),
        "hg_tri_kernel_names": (C.c_char_p, []),
        "hg_tri_launch_counts": (u32, [vp, u32]),
    }
    return _load("libhypergen_tri.so", TRI_LIB_PATH, sig, TRI_EXPORTS)


def tri_text_bytes(layout, row0, rows, cols):
    """hg_tri_text_bytes (needs no GPU): the bytes of the field text of the rows [row0, row0 + rows)"""
    return int(lib_tri().hg_tri_text_bytes(layout, row0, rows, cols))


def tri_field_offset(layout, row0, i, j, cols):
    """hg_tri_field_offset (needs no GPU): where the field of the pair (i, j) starts in the field text of a block at row0"""
    return int(lib_tri().hg_tri_field_offset(layout, row0, i, j, cols))


def tri_geometry():
    """dict of hg_tri_tile_rows, hg_tri_tile_cols and hg_tri_threads"""
    L = lib_tri()
    return {"tile_rows": int(L.hg_tri_tile_rows()), "tile_cols": int(L.hg_tri_tile_cols()), "threads": int(L.hg_tri_threads())}


def tri_kernel_names():
    """hg_tri_kernel_names: the library's kernels as rocprofv3 spells them"""
    return lib_tri().hg_tri_kernel_names().decode().split("\n")


def tri_launch_counts():
    """hg_tri_launch_counts: {kernel name: launches of this process so far}"""
    names = tri_kernel_names()
    counts = np.zeros(len(names), np.uint64)
    assert lib_tri().hg_tri_launch_counts(_ptr(counts), counts.size) == len(names)
    return dict(zip(names, (int(x) for x in counts)))


def dist_tile_order(tiles_m, tiles_n, tile_rows=256, tile_cols=320, diagonal_first=False, symmetric=False, ref_off=0, qry_off=0):
    """hg_dist_tile_order: the slot -> tile table of a launch as a uint32 array (tm | tn << 16, 0xFFFFFFFF = no tile)"""
    n = C.c_size_t(0)
    st = lib().hg_dist_tile_order(tiles_m, tiles_n, tile_rows, tile_cols, int(diagonal_first), int(symmetric), ref_off, qry_off,
                                  None, 0, C.byref(n))
    if st not in (OK, ERR_CAPACITY):
        raise HgError(st, "hg_dist_tile_order")
    out = np.zeros(max(n.value, 1), np.uint32)
    st = lib().hg_dist_tile_order(tiles_m, tiles_n, tile_rows, tile_cols, int(diagonal_first), int(symmetric), ref_off, qry_off,
                                  C.c_void_p(out.ctypes.data), out.size, C.byref(n))
    if st != OK:
        raise HgError(st, "hg_dist_tile_order")
    return out[: n.value]


def default_params(**kw):
    """hg_sketch_params_default, then the fields given by name (min_count=2 keeps the sampled k-mers seen at least twice)."""
    p = SketchParams()
    lib().hg_sketch_params_default(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


# Harness-side defaults for hg_ctx_set_debug, applied to every Context created while they are set (the test-suite's
# "run this module in both input forms" switch: tests/conftest.py sets {"kmer_input": "packed"}).  The library itself
# reads neither this nor the environment.
default_debug = {}


class Context:
    """One device + stream + workspaces (hg_ctx).  Not thread-safe."""

    def __init__(self, device=0):
        self._h = C.c_void_p()
        st = lib().hg_ctx_create(device, C.byref(self._h))
        if st != OK:
            raise HgError(st, lib().hg_last_error(None).decode())
        for k, v in default_debug.items():
            self.set_debug(k, v)

    def close(self):
        if self._h:
            lib().hg_ctx_destroy(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, st, allow=()):
        if st != OK and st not in allow:
            raise HgError(st, lib().hg_last_error(self._h).decode())
        return st

    def set_stream(self, stream_handle):
        """Run on the given hipStream_t handle; 0 / None is HIP's default stream (torch's default current stream)."""
        self._ck(lib().hg_ctx_set_stream(self._h, C.c_void_p(stream_handle or 0)))

    def set_debug(self, key, value):
        """Development / test hook: force an internal code path of this ctx (hg_ctx_set_debug)."""
        self._ck(lib().hg_ctx_set_debug(self._h, key.encode(), str(value).encode()))

    def reset_stream(self):
        self._ck(lib().hg_ctx_reset_stream(self._h))

    def sync(self):
        """hg_ctx_sync: reads a queued sketch step's check word (re-running the step if it asks for it), then waits for the stream."""
        self._ck(lib().hg_ctx_sync(self._h))

    def logf_dev(self, d_out, n, d_x=None, first_bits=0):
        """hg_logf_dev: the library's logf of n floats (d_x), or of the bit patterns first_bits .. first_bits + n - 1"""
        self._ck(lib().hg_logf_dev(self._h, C.c_void_p(d_x or 0), first_bits, n, C.c_void_p(d_out)))

    def ani_from_dots_dev(self, d_dot, d_nr, d_nq, n, ksize, d_ani):
        self._ck(lib().hg_ani_from_dots_dev(self._h, C.c_void_p(d_dot), C.c_void_p(d_nr), C.c_void_p(d_nq), n, ksize, C.c_void_p(d_ani)))

    def sketch_step_counts(self):
        """(sync-free, synchronous, re-run) sketch steps of this ctx so far (hg_ctx_sketch_step_counts)."""
        a, b, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
        self._ck(lib().hg_ctx_sketch_step_counts(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return int(a.value), int(b.value), int(c.value)

    def last_kernel(self, cls):
        """Name of the kernel the last call launched for a timing class ("kmer", "dist"), as rocprofv3 prints it; for "sort" and
        "encode" every kernel the last sketch step queued for the class, in launch order, joined by " + "."""
        return lib().hg_ctx_last_kernel(self._h, T_NAMES.index(cls)).decode()

    def enable_timing(self, on=True):
        self._ck(lib().hg_ctx_enable_timing(self._h, int(on)))

    def timings(self):
        """{kernel class: (sum of launch durations in ms, launches)} since the last call."""
        ms = (C.c_float * T_COUNT)()
        n = (C.c_uint32 * T_COUNT)()
        self._ck(lib().hg_ctx_timings(self._h, ms, n))
        return {name: (float(ms[i]), int(n[i])) for i, name in enumerate(T_NAMES)}

    # ---- host-buffer entry points -----------------------------------------------------------
    def _hash_sample(self, call, seq, scaled, threshold, cap, per_start=1):
        """call(seq pointer, seq bytes, threshold, out pointer, cap, byref(n)) -> status, with an output that grows to what
        the call asks for while it returns ERR_CAPACITY; the default capacity allows for per_start k-mers per start"""
        a = _u8(seq)
        thr = (2**64 - 1) // scaled if threshold is None else threshold
        cap = cap if cap is not None else max(1024, per_start * a.size // max(1, scaled) * 2 + 1024)
        while True:
            out = np.zeros(max(cap, 1), np.uint64)
            n = C.c_size_t(0)
            st = call(_ptr(a) if a.size else None, a.size, C.c_uint64(thr), _ptr(out), cap, C.byref(n))
            if st == ERR_CAPACITY:
                cap = n.value
                continue
            self._ck(st)
            return out[: n.value].copy()

    def kmer_hash_sample(self, seq, ksize=21, scaled=1500, seed=123, canonical=True,
                         norm=NORM_ACGT, threshold=None, cap=None, min_count=1):
        """The distinct sampled hashes, ascending; min_count > 1: those that occur at least that often (hg_kmer_hash_sample_min_count)."""
        fn, more = (lib().hg_kmer_hash_sample_min_count, (min_count,)) if min_count > 1 else (lib().hg_kmer_hash_sample, ())
        return self._hash_sample(lambda a, n, thr, *out: fn(self._h, a, n, ksize, thr, C.c_uint64(seed), int(canonical), norm, *more, *out),
                                 seq, scaled, threshold, cap)

    def unpack2_dev(self, d_blob, n_bps, d_out):
        """hg_unpack2_dev on device pointers (ints)"""
        self._ck(lib().hg_unpack2_dev(self._h, C.c_void_p(d_blob), n_bps, C.c_void_p(d_out)))

    def hv_encode(self, hashes, hv_d=4096, layout=LAYOUT_AVX2):
        h = np.ascontiguousarray(hashes, dtype=np.uint64)
        hv = np.zeros(hv_d, np.int16)
        n2 = C.c_int32(0)
        self._ck(lib().hg_hv_encode(self._h, _ptr(h) if h.size else None, h.size, hv_d, layout,
                                    _ptr(hv), C.byref(n2)))
        return hv, int(n2.value)

    def sketch_batch(self, seqs, params=None):
        return _sketch_batch_host(self._ck, lib().hg_sketch_batch, self._h, seqs, params or default_params())

    # ---- amino-acid k-mers (libhypergen_aa.so) ----------------------------------------------
    def aa_hash_sample(self, seq, ksize=9, scaled=1500, seed=123, threshold=None, cap=None):
        """hg_aa_hash_sample: the distinct sampled hashes of a residue sequence, ascending"""
        return self._hash_sample(lambda a, n, thr, *out: lib_aa().hg_aa_hash_sample(self._h, a, n, ksize, thr, C.c_uint64(seed), *out),
                                 seq, scaled, threshold, cap)

    def aa_sketch_batch(self, seqs, params=None):
        """hg_aa_sketch_batch: (hv, norm2, nhash) of host proteomes"""
        return _sketch_batch_host(self._ck, lib_aa().hg_aa_sketch_batch, self._h, seqs, params or default_params(ksize=9))

    def aa_sketch_batch_dev(self, d_seq, offsets, lens, params, d_hv, d_norm2, d_nhash):
        """hg_aa_sketch_batch_dev on device pointers (ints); final in stream order"""
        self._sketch_batch_dev(lib_aa().hg_aa_sketch_batch_dev, d_seq, offsets, lens, params, d_hv, d_norm2, d_nhash)

    # ---- six-frame translated k-mers (libhypergen_tx.so) -------------------------------------
    def tx_hash_sample(self, seq, ksize=9, scaled=1500, seed=123, threshold=None, cap=None):
        """hg_tx_hash_sample: the distinct sampled hashes of the six frames of a nucleotide sequence, ascending"""
        return self._hash_sample(lambda a, n, thr, *out: lib_tx().hg_tx_hash_sample(self._h, a, n, ksize, thr, C.c_uint64(seed), *out),
                                 seq, scaled, threshold, cap, per_start=2)

    def tx_plan_regrows(self):
        """hg_tx_plan_regrows: how often this ctx's synchronous sketch path rebuilt a plan after a hit region overflowed"""
        return int(lib_tx().hg_tx_plan_regrows(self._h))

    def tx_sketch_batch(self, seqs, params=None):
        """hg_tx_sketch_batch: (hv, norm2, nhash) of host genomes (ASCII)"""
        return _sketch_batch_host(self._ck, lib_tx().hg_tx_sketch_batch, self._h, seqs, params or default_params(ksize=9))

    def tx_sketch_batch_dev(self, d_seq, offsets, lens, params, d_hv, d_norm2, d_nhash):
        """hg_tx_sketch_batch_dev on device pointers (ints); final in stream order"""
        self._sketch_batch_dev(lib_tx().hg_tx_sketch_batch_dev, d_seq, offsets, lens, params, d_hv, d_norm2, d_nhash)

    # ---- one multi-FASTA text into records (libhypergen_rec.so) --------------------------------
    def rec_count_dev(self, d_text, n):
        """hg_rec_count_dev on a device pointer (int): (status, n_recs, seq_bytes); raises unless OK or HG_ERR_IO"""
        n_recs, seq_bytes = C.c_size_t(0), C.c_size_t(0)
        st = self._ck(lib_rec().hg_rec_count_dev(self._h, _ptr(d_text), n, C.byref(n_recs), C.byref(seq_bytes)), allow=(ERR_IO,))
        return st, int(n_recs.value), int(seq_bytes.value)

    def rec_split_dev(self, d_text, n, d_seq, seq_cap, d_recs, rec_cap):
        """hg_rec_split_dev on device pointers (ints): (status, n_recs, seq_bytes); raises unless OK, HG_ERR_IO or HG_ERR_CAPACITY"""
        n_recs, seq_bytes = C.c_size_t(0), C.c_size_t(0)
        st = self._ck(lib_rec().hg_rec_split_dev(self._h, _ptr(d_text), n, _ptr(d_seq), seq_cap, _ptr(d_recs), rec_cap,
                                                 C.byref(n_recs), C.byref(seq_bytes)), allow=(ERR_IO, ERR_CAPACITY))
        return st, int(n_recs.value), int(seq_bytes.value)

    def rec_split(self, text, seq_cap=None, rec_cap=None, fill=0xEE):
        """hg_rec_split, host memory in and out, with the arguments and results of rec_split_host()"""
        def fn(*a):
            return self._ck(lib_rec().hg_rec_split(self._h, *a), allow=(ERR_IO, ERR_CAPACITY))
        return _sized_then_called(lambda sc, rc: _rec_host_call(fn, text, sc, rc, fill), seq_cap, rec_cap)

    def rec_sketch_text_dev(self, d_text, n, params, min_length=0):
        """hg_rec_sketch_text_dev on a device pointer (int): (record table, indices of the sketched records, hv, norm2, nhash),
        the rows in the order of the indices"""
        got = {"recs": np.zeros(0, REC_DTYPE), "which": [], "hv": [], "n2": [], "nh": [], "calls": 0}

        def rows(user, recs, n_recs, which, m, hv, n2, nh):
            got["calls"] += 1
            if m == 0:
                got["recs"] = np.frombuffer(C.string_at(recs, n_recs * REC_DTYPE.itemsize), REC_DTYPE).copy()
                return 0
            got["which"].append(np.frombuffer(C.string_at(which, m * 4), np.uint32).copy())
            got["hv"].append(np.frombuffer(C.string_at(hv, m * params.hv_d * 2), np.int16).reshape(m, params.hv_d).copy())
            got["n2"].append(np.frombuffer(C.string_at(n2, m * 4), np.int32).copy())
            got["nh"].append(np.frombuffer(C.string_at(nh, m * 4), np.uint32).copy())
            return 0

        n_recs, n_kept = C.c_size_t(0), C.c_size_t(0)
        self._ck(lib_rec().hg_rec_sketch_text_dev(self._h, _ptr(d_text), n, C.byref(params), C.c_uint64(min_length), REC_ROWS_FN(rows), None,
                                                  C.byref(n_recs), C.byref(n_kept)))
        assert got["recs"].size == n_recs.value
        which = np.concatenate(got["which"]) if got["which"] else np.zeros(0, np.uint32)
        assert which.size == n_kept.value
        hv = np.concatenate(got["hv"]) if got["hv"] else np.zeros((0, params.hv_d), np.int16)
        n2 = np.concatenate(got["n2"]) if got["n2"] else np.zeros(0, np.int32)
        nh = np.concatenate(got["nh"]) if got["nh"] else np.zeros(0, np.uint32)
        return got["recs"], which, hv, n2, nh

    # ---- fragment-wise ANI and aligned fraction (libhypergen_frag.so) --------------------------
    def frag_sketch_seq_dev(self, d_seq, n_bps, params, window, step):
        """hg_frag_sketch_seq_dev on a device pointer (int): (starts, lens, hv, norm2, nhash) of the planned windows, in order"""
        got = {"starts": [], "lens": [], "hv": [], "n2": [], "nh": [], "next": 0}

        def rows(user, starts, lens, first, m, hv, n2, nh):
            if first != got["next"]:
                return 1
            got["next"] += m
            got["starts"].append(np.frombuffer(C.string_at(starts, m * 8), np.uint64).copy())
            got["lens"].append(np.frombuffer(C.string_at(lens, m * 8), np.uint64).copy())
            got["hv"].append(np.frombuffer(C.string_at(hv, m * params.hv_d * 2), np.int16).reshape(m, params.hv_d).copy())
            got["n2"].append(np.frombuffer(C.string_at(n2, m * 4), np.int32).copy())
            got["nh"].append(np.frombuffer(C.string_at(nh, m * 4), np.uint32).copy())
            return 0

        n_windows = C.c_size_t(0)
        self._ck(lib_frag().hg_frag_sketch_seq_dev(self._h, _ptr(d_seq), n_bps, C.byref(params), window, step, FRAG_ROWS_FN(rows), None,
                                                   C.byref(n_windows)))
        assert got["next"] == n_windows.value
        return tuple(np.concatenate(got[k]) for k in ("starts", "lens", "hv", "n2", "nh"))

    def frag_ani_matrix_dev(self, d_ani, R, Q, ref_first, qry_first, frag_th, d_pair, d_best=None, allow=()):
        """hg_frag_ani_matrix_dev on device pointers (ints); the offsets are host arrays of n + 1 entries.  Returns the status."""
        rf, n_ref = _frag_offsets(ref_first)
        qf, n_qry = _frag_offsets(qry_first)
        return self._ck(lib_frag().hg_frag_ani_matrix_dev(self._h, _ptr(d_ani), R, Q, _ptr(rf) if rf.size else None, n_ref,
                                                          _ptr(qf) if qf.size else None, n_qry, frag_th, _ptr(d_pair),
                                                          _ptr(d_best) if d_best is not None else None), allow=allow)

    def frag_ani_dev(self, d_ref, d_rn, R, d_qry, d_qn, Q, hv_d, ksize, ref_first, qry_first, frag_th, d_pair, d_best=None, block_rows=0,
                     allow=()):
        """hg_frag_ani_dev on device pointers (ints), under the ctx's ANI metric.  Returns the status."""
        rf, n_ref = _frag_offsets(ref_first)
        qf, n_qry = _frag_offsets(qry_first)
        return self._ck(lib_frag().hg_frag_ani_dev(self._h, _ptr(d_ref), _ptr(d_rn), R, _ptr(d_qry), _ptr(d_qn), Q, hv_d, ksize,
                                                   _ptr(rf) if rf.size else None, n_ref, _ptr(qf) if qf.size else None, n_qry, frag_th,
                                                   block_rows, _ptr(d_pair), _ptr(d_best) if d_best is not None else None), allow=allow)

    def frag_ani(self, ref_hv, ref_n2, qry_hv, qry_n2, ref_first, qry_first, frag_th, ksize=21, want_best=True):
        """hg_frag_ani, host arrays in and out: (pair records [n_ref, n_qry], best records [n_ref, Q] or None)"""
        r, q = np.ascontiguousarray(ref_hv, np.int16), np.ascontiguousarray(qry_hv, np.int16)
        rn, qn = np.ascontiguousarray(ref_n2, np.int32), np.ascontiguousarray(qry_n2, np.int32)
        rf, n_ref = _frag_offsets(ref_first)
        qf, n_qry = _frag_offsets(qry_first)
        pair = np.zeros((n_ref, n_qry), FRAG_PAIR_DTYPE)
        best = np.zeros((n_ref, q.shape[0]), FRAG_BEST_DTYPE) if want_best else None
        self._ck(lib_frag().hg_frag_ani(self._h, _ptr(r), _ptr(rn), r.shape[0], _ptr(q), _ptr(qn), q.shape[0], r.shape[1], ksize,
                                        _ptr(rf) if rf.size else None, n_ref, _ptr(qf) if qf.size else None, n_qry, frag_th,
                                        _ptr(pair), _ptr(best) if want_best else None))
        return pair, best

    # ---- the histogram of the ANI values of a comparison (libhypergen_hist.so) ------------------
    def hist_add_matrix_dev(self, d_ani, rows, cols, pitch, row0, col0, pairs, bin_milli, d_counts, allow=()):
        """hg_hist_add_matrix_dev on device pointers (ints): ADDS the block's selected pairs to d_counts, in stream order.
        Returns the status."""
        return self._ck(lib_hist().hg_hist_add_matrix_dev(self._h, _ptr(d_ani), rows, cols, pitch, row0, col0, pairs, bin_milli,
                                                          _ptr(d_counts)), allow=allow)

    def hist_dev(self, d_ref, d_rn, R, d_qry, d_qn, Q, hv_d, ksize, pairs, bin_milli, d_counts, block_rows=0, allow=()):
        """hg_hist_dev on device pointers (ints), under the ctx's ANI metric; d_counts is zeroed first.  Returns the status."""
        return self._ck(lib_hist().hg_hist_dev(self._h, _ptr(d_ref), _ptr(d_rn), R, _ptr(d_qry), _ptr(d_qn), Q, hv_d, ksize, pairs,
                                               bin_milli, block_rows, _ptr(d_counts)), allow=allow)

    def hist(self, ref_hv, ref_n2, qry_hv=None, qry_n2=None, pairs=HIST_ALL, bin_milli=100, ksize=21):
        """hg_hist, host arrays in, the uint64 counts out; without a query side the reference set is compared with itself
        (the form HIST_UPPER and HIST_OFFDIAG need)"""
        r, rn = np.ascontiguousarray(ref_hv, np.int16), np.ascontiguousarray(ref_n2, np.int32)
        q, qn = (r, rn) if qry_hv is None else (np.ascontiguousarray(qry_hv, np.int16), np.ascontiguousarray(qry_n2, np.int32))
        counts = np.zeros(max(hist_bins(bin_milli), 1), np.uint64)
        self._ck(lib_hist().hg_hist(self._h, _ptr(r), _ptr(rn), r.shape[0], _ptr(q), _ptr(qn), q.shape[0], r.shape[1], ksize, pairs,
                                    bin_milli, _ptr(counts)))
        return counts

    # ---- the ANI matrix of all pairs as fixed-width text (libhypergen_tri.so) ------------------------
    def tri_format_dev(self, d_ani, rows, cols, pitch, row0, layout, d_text, allow=()):
        """hg_tri_format_dev on device pointers (ints): the fields of one block into d_text, in stream order.  Returns the status."""
        return self._ck(lib_tri().hg_tri_format_dev(self._h, _ptr(d_ani), rows, cols, pitch, row0, layout, _ptr(d_text)), allow=allow)

    def tri_dev(self, d_hv, d_n2, n, hv_d, ksize, layout, d_text, block_rows=0, allow=()):
        """hg_tri_dev on device pointers (ints), under the ctx's ANI metric: the whole field text into d_text.  Returns the status."""
        return self._ck(lib_tri().hg_tri_dev(self._h, _ptr(d_hv), _ptr(d_n2), n, hv_d, ksize, layout, block_rows, _ptr(d_text)), allow=allow)

    def tri_stream_dev(self, d_hv, d_n2, n, hv_d, ksize, layout, sink, block_rows=0, allow=()):
        """hg_tri_stream_dev on device pointers (ints): sink(text: bytes, row0, rows) is called per block on this thread and
        ends the call (HG_ERR_IO) by returning anything but None or 0.  Returns the status."""
        def c_sink(_user, text, nbytes, row0, rows):
            return int(sink(C.string_at(text, nbytes) if nbytes else b"", int(row0), int(rows)) or 0)

        return self._ck(lib_tri().hg_tri_stream_dev(self._h, _ptr(d_hv), _ptr(d_n2), n, hv_d, ksize, layout, block_rows, TRI_SINK(c_sink), None),
                        allow=allow)

    def tri(self, hv, n2, layout=TRI_LOWER, ksize=21):
        """hg_tri, host arrays in, the field text of all pairs of the set out (bytes)"""
        h, hn = np.ascontiguousarray(hv, np.int16), np.ascontiguousarray(n2, np.int32)
        n = h.shape[0]
        text = np.zeros(max(tri_text_bytes(layout, 0, n, n), 1), np.uint8)
        self._ck(lib_tri().hg_tri(self._h, _ptr(h), _ptr(hn), n, h.shape[1], ksize, layout, _ptr(text)))
        return text[: tri_text_bytes(layout, 0, n, n)].tobytes()

    def dist_full(self, ref_hv, ref_n2, qry_hv, qry_n2, ksize=21):
        r = np.ascontiguousarray(ref_hv, np.int16)
        q = np.ascontiguousarray(qry_hv, np.int16)
        rn = np.ascontiguousarray(ref_n2, np.int32)
        qn = np.ascontiguousarray(qry_n2, np.int32)
        out = np.zeros((r.shape[0], q.shape[0]), np.float32)
        self._ck(lib().hg_dist_full(self._h, _ptr(r), _ptr(rn), r.shape[0], _ptr(q), _ptr(qn),
                                    q.shape[0], r.shape[1], ksize, _ptr(out)))
        return out

    def dist(self, ref_hv, ref_n2, qry_hv, qry_n2, ksize=21, symmetric=False, ani_th=85.0, cap=None):
        r = np.ascontiguousarray(ref_hv, np.int16)
        q = np.ascontiguousarray(qry_hv, np.int16)
        rn = np.ascontiguousarray(ref_n2, np.int32)
        qn = np.ascontiguousarray(qry_n2, np.int32)
        cap = cap if cap is not None else max(1024, r.shape[0] * q.shape[0] // 8)
        while True:
            out = np.zeros(cap, ANI_HIT_DTYPE)
            n = C.c_size_t(0)
            st = lib().hg_dist(self._h, _ptr(r), _ptr(rn), r.shape[0], _ptr(q), _ptr(qn), q.shape[0],
                               r.shape[1], ksize, int(symmetric), C.c_float(ani_th), _ptr(out), cap,
                               C.byref(n))
            if st == ERR_CAPACITY:
                cap = n.value
                continue
            self._ck(st)
            return out[: n.value].copy()

    # ---- device-resident entry points (pointers are ints, e.g. torch.Tensor.data_ptr()) -------
    def _sketch_batch_dev(self, fn, d_seq, offsets, lens, params, d_hv, d_norm2, d_nhash):
        off = np.ascontiguousarray(offsets, np.uint64)
        ln = np.ascontiguousarray(lens, np.uint64)
        self._ck(fn(self._h, _ptr(d_seq), _ptr(off), _ptr(ln), off.size, C.byref(params), _ptr(d_hv), _ptr(d_norm2), _ptr(d_nhash)))

    def sketch_batch_dev(self, d_seq, offsets, lens, params, d_hv, d_norm2, d_nhash):
        self._sketch_batch_dev(lib().hg_sketch_batch_dev, d_seq, offsets, lens, params, d_hv, d_norm2, d_nhash)

    def sketch_batch_dev_packed(self, d_blobs, offsets, n_bps, params, d_hv, d_norm2, d_nhash):
        """hg_sketch_batch_dev_packed: genome i is the hg_pack2 blob at d_blobs + offsets[i] (multiples of 16)"""
        self._sketch_batch_dev(lib().hg_sketch_batch_dev_packed, d_blobs, offsets, n_bps, params, d_hv, d_norm2, d_nhash)

    def pack2_batch_dev(self, d_seq, offsets, lens, d_blobs, blob_offsets, norm_mode=NORM_ACGT):
        """hg_pack2_batch_dev: ASCII genomes resident in HBM -> hg_pack2 blobs (device pointers are ints)"""
        off = np.ascontiguousarray(offsets, np.uint64)
        ln = np.ascontiguousarray(lens, np.uint64)
        bo = np.ascontiguousarray(blob_offsets, np.uint64)
        self._ck(lib().hg_pack2_batch_dev(self._h, _ptr(d_seq), _ptr(off), _ptr(ln), off.size, norm_mode, _ptr(d_blobs), _ptr(bo)))

    def pack2_dev(self, d_seq, n_bps, d_blob, norm_mode=NORM_ACGT):
        self._ck(lib().hg_pack2_dev(self._h, C.c_void_p(d_seq), n_bps, norm_mode, C.c_void_p(d_blob)))

    def synth_genomes_dev(self, first, n, L, stride, d_out, cluster_size=100, sub_ppm_per_member=1000):
        done = 0
        while done < n:  # grid.y limit
            m = min(n - done, 32768)
            self._ck(lib().hg_synth_genomes_dev(self._h, first + done, m, L, cluster_size, sub_ppm_per_member,
                                                stride, C.c_void_p(int(d_out) + done * stride)))
            done += m

    # ---- bit-packed extension (device pointers) ---------------------------------------------------
    def hv_binarize_dev(self, d_hv, n, hv_d, d_bits):
        self._ck(lib().hg_hv_binarize_dev(self._h, _ptr(d_hv), n, hv_d, _ptr(d_bits)))

    def hamming_full_dev(self, d_ref, R, d_qry, Q, hv_d, d_out):
        self._ck(lib().hg_hamming_full_dev(self._h, _ptr(d_ref), R, _ptr(d_qry), Q, hv_d, _ptr(d_out)))

    def hamming_search_dev(self, d_ref, R, d_qry, Q, hv_d, max_dist, d_out, cap):
        n = C.c_size_t(0)
        st = lib().hg_hamming_search_dev(self._h, _ptr(d_ref), R, _ptr(d_qry), Q, hv_d, max_dist, _ptr(d_out), cap,
                                         C.byref(n))
        self._ck(st, allow=(ERR_CAPACITY,))
        return n.value, st

    def dist_full_dev(self, d_ref, d_rn, R, d_qry, d_qn, Q, hv_d, ksize, d_out):
        self._ck(lib().hg_dist_full_dev(self._h, _ptr(d_ref), _ptr(d_rn), R, _ptr(d_qry), _ptr(d_qn), Q,
                                        hv_d, ksize, _ptr(d_out)))

    def dist_block_dev(self, d_ref, d_rn, R, ref_off, d_qry, d_qn, Q, qry_off, hv_d, ksize, symmetric, ani_th,
                       d_out, cap):
        n = C.c_size_t(0)
        st = lib().hg_dist_block_dev(self._h, _ptr(d_ref), _ptr(d_rn), R, ref_off, _ptr(d_qry), _ptr(d_qn), Q,
                                     qry_off, hv_d, ksize, int(symmetric), C.c_float(ani_th), _ptr(d_out), cap,
                                     C.byref(n))
        self._ck(st, allow=(ERR_CAPACITY,))
        return n.value, st

    def dist_prep_ops_dev(self, d_hv, rows, hv_d, d_ops, d_meta, d_flag):
        """hg_dist_prep_ops_dev: byte operands + control records of this rank's reference rows (device pointers)"""
        self._ck(lib().hg_dist_prep_ops_dev(self._h, _ptr(d_hv), rows, hv_d, _ptr(d_ops), _ptr(d_meta), _ptr(d_flag)))

    def dist_block_ops_dev(self, d_ref_ops, d_ref_meta, d_rn, R, ref_off, d_ref_index, d_flags, n_flags, d_qry, d_qn, Q, qry_off,
                           hv_d, ksize, symmetric, ani_th, d_out, cap):
        """hg_dist_block_ops_dev; returns (hits, status) -- status ERR_INEXACT: vetoed, fall back to dist_block_dev"""
        n = C.c_size_t(0)
        st = lib().hg_dist_block_ops_dev(self._h, _ptr(d_ref_ops), _ptr(d_ref_meta), _ptr(d_rn), R, ref_off,
                                         _ptr(d_ref_index) if d_ref_index else None, _ptr(d_flags) if d_flags else None, n_flags,
                                         _ptr(d_qry), _ptr(d_qn), Q, qry_off, hv_d, ksize, int(symmetric), C.c_float(ani_th),
                                         _ptr(d_out), cap, C.byref(n))
        self._ck(st, allow=(ERR_CAPACITY, ERR_INEXACT))
        return n.value, st

    def hamming_search_block_dev(self, d_ref, R, ref_off, d_qry, Q, qry_off, hv_d, max_dist, d_out, cap):
        n = C.c_size_t(0)
        st = lib().hg_hamming_search_block_dev(self._h, _ptr(d_ref), R, ref_off, _ptr(d_qry), Q, qry_off, hv_d,
                                               max_dist, _ptr(d_out), cap, C.byref(n))
        self._ck(st, allow=(ERR_CAPACITY,))
        return n.value, st

    def hv_unpack_batch_dev(self, d_payloads, payloads_bytes, offsets, quant_bits, layouts, hv_d, d_hv):
        """decompress_file_sketch on the device: payload i at d_payloads + offsets[i] -> row i of d_hv (n x hv_d int16)"""
        offsets = np.ascontiguousarray(offsets, np.uint64)
        quant_bits = np.ascontiguousarray(quant_bits, np.uint8)
        lay = None if layouts is None else np.ascontiguousarray(layouts, np.uint8)
        self._ck(lib().hg_hv_unpack_batch_dev(self._h, d_payloads, payloads_bytes, _ptr(offsets), _ptr(quant_bits),
                                              None if lay is None else _ptr(lay), offsets.size, hv_d, d_hv))

    def last_dist_path(self):
        """0 = f16 MFMA, 1 = i8 MFMA, 2 = integer VALU (all exact), -1 = no thresholded dist call yet."""
        return int(lib().hg_ctx_last_dist_path(self._h))

    def set_ani_metric(self, metric):
        """ANI_MASH (default), ANI_CONTAINMENT (dot / the query's norm: directional) or ANI_MAX_CONTAINMENT (dot / the
        smaller norm) for this ctx's later dist / cluster calls (hg_ctx_set_ani_metric)."""
        self._ck(lib().hg_ctx_set_ani_metric(self._h, metric))

    def ani_metric(self):
        return int(lib().hg_ctx_ani_metric(self._h))

    def last_hamming_path(self):
        """0 = xor + popcount kernel, 1 = +-1 byte GEMM on the matrix pipe (same integers), -1 = none yet."""
        return int(lib().hg_ctx_last_hamming_path(self._h))

    def sort_ani_hits_dev(self, d_hits, n, Q):
        self._ck(lib().hg_sort_ani_hits_dev(self._h, _ptr(d_hits), n, Q))

    def sort_ani_hits_staged(self, hits, Q):
        hits = np.ascontiguousarray(hits, ANI_HIT_DTYPE).copy()
        self._ck(lib().hg_sort_ani_hits_staged(self._h, _ptr(hits), hits.size, Q))
        return hits

    def topk_per_query_dev(self, d_hits, n, Q, k, d_out, d_counts):
        self._ck(lib().hg_topk_per_query_dev(self._h, _ptr(d_hits), n, Q, k, _ptr(d_out), _ptr(d_counts)))

    def search_topk_dev(self, d_ref, d_rn, R, d_qry, d_qn, Q, hv_d, ksize, ani_th, k, d_out, d_counts, ref_off=0, qry_off=0):
        """hg_search_topk_block_dev (hg_search_topk_dev with both offsets 0): per query the k best references with
        ani >= ani_th into d_out (Q * k hits, the layout of topk_per_query_dev) and d_counts; device pointers, stream-ordered."""
        self._ck(lib().hg_search_topk_block_dev(self._h, _ptr(d_ref), _ptr(d_rn), R, ref_off, _ptr(d_qry), _ptr(d_qn), Q, qry_off,
                                                hv_d, ksize, C.c_float(ani_th), k, _ptr(d_out), _ptr(d_counts)))

    def search_topk(self, ref_hv, ref_n2, qry_hv, qry_n2, ksize=21, ani_th=85.0, k=1):
        """hg_search_topk on host sketches: (hits of shape (Q, k) with ANI_HIT_DTYPE, counts)"""
        r = np.ascontiguousarray(ref_hv, np.int16)
        q = np.ascontiguousarray(qry_hv, np.int16)
        rn = np.ascontiguousarray(ref_n2, np.int32)
        qn = np.ascontiguousarray(qry_n2, np.int32)
        out = np.zeros((q.shape[0], k), ANI_HIT_DTYPE)
        cnt = np.zeros(q.shape[0], np.uint32)
        self._ck(lib().hg_search_topk(self._h, _ptr(r) if r.size else None, _ptr(rn) if rn.size else None, r.shape[0], _ptr(q),
                                      _ptr(qn), q.shape[0], q.shape[1], ksize, C.c_float(ani_th), k, _ptr(out), _ptr(cnt)))
        return out, cnt

    def ani_pairs_dev(self, d_ref, d_rn, R, d_qry, d_qn, Q, hv_d, ksize, d_pairs, n_pairs, columns, d_ani, d_dot=None):
        """hg_ani_pairs_dev: the `columns` (PAIRS_* mask) of the n_pairs listed pairs into d_ani (n_pairs x popcount(columns)
        floats), their wrapped i32 dots into d_dot if given; device pointers, results final on return."""
        self._ck(lib().hg_ani_pairs_dev(self._h, _ptr(d_ref), _ptr(d_rn), R, _ptr(d_qry), _ptr(d_qn), Q, hv_d, ksize,
                                        _ptr(d_pairs or 0), n_pairs, columns, _ptr(d_ani or 0), _ptr(d_dot or 0)))  # (None / 0: NULL)

    def ani_pairs(self, ref_hv, ref_n2, qry_hv, qry_n2, pairs, columns, ksize=21, want_dot=False):
        """hg_ani_pairs on host sketches.  pairs: an ANI_HIT_DTYPE array (its `ani` is ignored) or an (n, 2) integer array of
        (ref_idx, qry_idx).  Returns the (n, popcount(columns)) float32 array, with want_dot (array, int32 dots)."""
        r = np.ascontiguousarray(ref_hv, np.int16)
        q = r if qry_hv is ref_hv else np.ascontiguousarray(qry_hv, np.int16)
        rn = np.ascontiguousarray(ref_n2, np.int32)
        qn = rn if qry_n2 is ref_n2 else np.ascontiguousarray(qry_n2, np.int32)
        pairs = np.asarray(pairs)
        if pairs.dtype != ANI_HIT_DTYPE:
            ij = pairs.reshape(-1, 2)
            pairs = np.zeros(ij.shape[0], ANI_HIT_DTYPE)
            pairs["ref_idx"], pairs["qry_idx"] = ij[:, 0], ij[:, 1]
        pairs = np.ascontiguousarray(pairs.ravel())
        n = pairs.size
        ani = np.zeros((n, bin(columns).count("1")), np.float32)
        dot = np.zeros(n, np.int32) if want_dot else None
        self._ck(lib().hg_ani_pairs(self._h, _ptr(r), _ptr(rn), r.shape[0], _ptr(q), _ptr(qn), q.shape[0], r.shape[1], ksize,
                                    _ptr(pairs) if n else None, n, columns, _ptr(ani) if ani.size else None,
                                    _ptr(dot) if want_dot and n else None))
        return (ani, dot) if want_dot else ani

    def dist_dev(self, d_ref, d_rn, R, d_qry, d_qn, Q, hv_d, ksize, symmetric, ani_th, d_out, cap):
        n = C.c_size_t(0)
        st = lib().hg_dist_dev(self._h, _ptr(d_ref), _ptr(d_rn), R, _ptr(d_qry), _ptr(d_qn), Q, hv_d,
                               ksize, int(symmetric), C.c_float(ani_th), _ptr(d_out), cap, C.byref(n))
        self._ck(st, allow=(ERR_CAPACITY,))
        return n.value, st

    # ---- single-linkage clustering (hg_cluster*) --------------------------------------------------
    def cluster(self, hv, n2, ksize=21, ani_th=95.0):
        """hg_cluster on host sketches: numpy (rep, cluster, n_clusters) -- rep[i] = smallest index of i's component,
        cluster[i] = its dense id in order of rep"""
        h = np.ascontiguousarray(hv, np.int16)
        nn = np.ascontiguousarray(n2, np.int32)
        n = h.shape[0]
        rep = np.zeros(n, np.uint32)
        cl = np.zeros(n, np.uint32)
        nc = C.c_size_t(0)
        self._ck(lib().hg_cluster(self._h, _ptr(h), _ptr(nn), n, h.shape[1], ksize, C.c_float(ani_th),
                                  _ptr(rep), _ptr(cl), C.byref(nc)))
        return rep, cl, nc.value

    def cluster_dev(self, d_hv, d_n2, n, hv_d, d_rep, d_cluster, ksize=21, ani_th=95.0):
        """hg_cluster_dev on resident sketches (device pointers); returns the number of clusters"""
        nc = C.c_size_t(0)
        self._ck(lib().hg_cluster_dev(self._h, _ptr(d_hv), _ptr(d_n2), n, hv_d, ksize, C.c_float(ani_th), _ptr(d_rep),
                                      _ptr(d_cluster), C.byref(nc)))
        return nc.value

    def cluster_init_dev(self, d_rep, n):
        self._ck(lib().hg_cluster_init_dev(self._h, _ptr(d_rep), n))

    def cluster_add_hits_dev(self, d_rep, n, d_hits, n_hits, ani_th):
        self._ck(lib().hg_cluster_add_hits_dev(self._h, _ptr(d_rep), n, _ptr(d_hits), n_hits, C.c_float(ani_th)))

    def cluster_finish_dev(self, d_rep, n, d_cluster):
        """returns the number of clusters; raises HgError(ERR_INVALID) if a hit since the init had an index >= n"""
        nc = C.c_size_t(0)
        self._ck(lib().hg_cluster_finish_dev(self._h, _ptr(d_rep), n, _ptr(d_cluster), C.byref(nc)))
        return nc.value

    # ---- the three forms of a representative scheme (greedy, set cover), given its C function ----------
    def _rep_host(self, fn, hv, n2, ksize, ani_th):
        h = np.ascontiguousarray(hv, np.int16)
        nn = np.ascontiguousarray(n2, np.int32)
        n = h.shape[0]
        rep = np.zeros(n, np.uint32)
        cl = np.zeros(n, np.uint32)
        ani = np.zeros(n, np.float32)
        nc = C.c_size_t(0)
        self._ck(fn(self._h, _ptr(h), _ptr(nn), n, h.shape[1], ksize, C.c_float(ani_th), _ptr(rep), _ptr(cl), _ptr(ani), C.byref(nc)))
        return rep, cl, ani, nc.value

    def _rep_dev(self, fn, d_hv, d_n2, n, hv_d, d_rep, d_cluster, d_ani, ksize, ani_th):
        nc = C.c_size_t(0)
        self._ck(fn(self._h, _ptr(d_hv), _ptr(d_n2), n, hv_d, ksize, C.c_float(ani_th), _ptr(d_rep), _ptr(d_cluster), _ptr(d_ani or 0),
                    C.byref(nc)))
        return nc.value

    def _rep_hits_dev(self, fn, n, d_hits, n_hits, ani_th, d_rep, d_cluster, d_ani):
        nc = C.c_size_t(0)
        self._ck(fn(self._h, n, _ptr(d_hits or 0), n_hits, C.c_float(ani_th), _ptr(d_rep or 0), _ptr(d_cluster or 0), _ptr(d_ani or 0),
                    C.byref(nc)))
        return nc.value

    # ---- greedy representative clustering (hg_cluster_greedy*) -----------------------------------
    def cluster_greedy(self, hv, n2, ksize=21, ani_th=95.0):
        """hg_cluster_greedy on host sketches in processing order: numpy (rep, cluster, ani, n_clusters) -- rep[i] = i for a
        representative, else the earlier representative with the highest ANI; cluster[i] = the dense id of rep[i];
        ani[i] = 100 for a representative, else the ANI of (rep[i], i)"""
        return self._rep_host(lib().hg_cluster_greedy, hv, n2, ksize, ani_th)

    def cluster_greedy_dev(self, d_hv, d_n2, n, hv_d, d_rep, d_cluster, d_ani=None, ksize=21, ani_th=95.0):
        """hg_cluster_greedy_dev on resident sketches (device pointers; d_ani may be None); returns the number of clusters"""
        return self._rep_dev(lib().hg_cluster_greedy_dev, d_hv, d_n2, n, hv_d, d_rep, d_cluster, d_ani, ksize, ani_th)

    def cluster_greedy_hits_dev(self, n, d_hits, n_hits, ani_th, d_rep, d_cluster, d_ani=None):
        """hg_cluster_greedy_hits_dev on a complete device-resident hit list (d_ani may be None); returns the number of
        clusters; raises HgError(ERR_INVALID) if a hit has an index >= n"""
        return self._rep_hits_dev(lib().hg_cluster_greedy_hits_dev, n, d_hits, n_hits, ani_th, d_rep, d_cluster, d_ani)

    def cluster_greedy_rounds(self):
        """rounds of the last greedy call on this ctx, summed over its blocks (hg_ctx_cluster_greedy_rounds)"""
        return int(lib().hg_ctx_cluster_greedy_rounds(self._h))

    # ---- greedy set-cover clustering (hg_cluster_setcover*) ---------------------------------------
    def cluster_setcover(self, hv, n2, ksize=21, ani_th=95.0):
        """hg_cluster_setcover on host sketches: numpy (rep, cluster, ani, n_clusters) -- the undecided sketch with the most
        undecided neighbours becomes a representative and takes them as its members, until none is left; rep[i] = i for a
        representative, else its representative; cluster[i] = the dense id of rep[i]; ani[i] = 100 for a
        representative, else the ANI of (rep[i], i)"""
        return self._rep_host(lib().hg_cluster_setcover, hv, n2, ksize, ani_th)

    def cluster_setcover_dev(self, d_hv, d_n2, n, hv_d, d_rep, d_cluster, d_ani=None, ksize=21, ani_th=95.0):
        """hg_cluster_setcover_dev on resident sketches (device pointers; d_ani may be None); returns the number of clusters"""
        return self._rep_dev(lib().hg_cluster_setcover_dev, d_hv, d_n2, n, hv_d, d_rep, d_cluster, d_ani, ksize, ani_th)

    def cluster_setcover_hits_dev(self, n, d_hits, n_hits, ani_th, d_rep, d_cluster, d_ani=None):
        """hg_cluster_setcover_hits_dev on a complete device-resident hit list (d_ani may be None); returns the number of
        clusters; raises HgError(ERR_INVALID) if a hit has an index >= n"""
        return self._rep_hits_dev(lib().hg_cluster_setcover_hits_dev, n, d_hits, n_hits, ani_th, d_rep, d_cluster, d_ani)

    def cluster_setcover_rounds(self):
        """rounds of the last set-cover call on this ctx (hg_ctx_cluster_setcover_rounds)"""
        return int(lib().hg_ctx_cluster_setcover_rounds(self._h))

    # ---- single-linkage tree (hg_cluster_tree*) ---------------------------------------------------
    def cluster_tree(self, hv, n2, ksize=21, ani_th=95.0, want_clusters=True):
        """hg_cluster_tree on host sketches: numpy (tree, rep, cluster, n_clusters) -- tree: the n - n_clusters edges
        {ref_idx = lo, qry_idx = hi, ani} of the maximum-ANI spanning forest at the floor ani_th, strongest first
        (ANI_HIT_DTYPE); rep / cluster as cluster() gives them at ani_th (None without want_clusters)"""
        h = np.ascontiguousarray(hv, np.int16)
        nn = np.ascontiguousarray(n2, np.int32)
        n = h.shape[0]
        tree = np.zeros(max(n, 1) - 1, ANI_HIT_DTYPE)
        rep = np.zeros(n, np.uint32) if want_clusters else None
        cl = np.zeros(n, np.uint32) if want_clusters else None
        ne, nc = C.c_size_t(0), C.c_size_t(0)
        keep = np.zeros(1, ANI_HIT_DTYPE)  # (a pointer that is not NULL for the empty tree of n <= 1)
        self._ck(lib().hg_cluster_tree(self._h, _ptr(h) if h.size else None, _ptr(nn) if nn.size else None, n,
                                       h.shape[1] if h.ndim == 2 else 0, ksize, C.c_float(ani_th),
                                       _ptr(tree if tree.size else keep), tree.size, C.byref(ne),
                                       _ptr(rep) if want_clusters and n else None, _ptr(cl) if want_clusters and n else None,
                                       C.byref(nc)))
        return tree[:ne.value], rep, cl, nc.value

    def cluster_tree_dev(self, d_hv, d_n2, n, hv_d, d_tree, tree_cap, d_rep=None, d_cluster=None, ksize=21, ani_th=95.0):
        """hg_cluster_tree_dev on resident sketches (device pointers; d_rep and d_cluster both given or both None); returns
        (n_edges, n_clusters).  HgError(ERR_CAPACITY) when tree_cap < n - 1"""
        ne, nc = C.c_size_t(0), C.c_size_t(0)
        self._ck(lib().hg_cluster_tree_dev(self._h, _ptr(d_hv or 0), _ptr(d_n2 or 0), n, hv_d, ksize, C.c_float(ani_th),
                                           _ptr(d_tree or 0), tree_cap, C.byref(ne), _ptr(d_rep or 0), _ptr(d_cluster or 0),
                                           C.byref(nc)))
        return ne.value, nc.value

    def cluster_tree_hits_dev(self, n, d_hits, n_hits, ani_th, d_tree, tree_cap, d_rep=None, d_cluster=None):
        """hg_cluster_tree_hits_dev on a complete device-resident hit list; returns (n_edges, n_clusters); raises
        HgError(ERR_INVALID) if a hit has an index >= n, HgError(ERR_CAPACITY) when tree_cap < n - 1"""
        ne, nc = C.c_size_t(0), C.c_size_t(0)
        self._ck(lib().hg_cluster_tree_hits_dev(self._h, n, _ptr(d_hits or 0), n_hits, C.c_float(ani_th), _ptr(d_tree or 0),
                                                tree_cap, C.byref(ne), _ptr(d_rep or 0), _ptr(d_cluster or 0), C.byref(nc)))
        return ne.value, nc.value

    def cluster_tree_rounds(self):
        """rounds of the last tree call on this ctx, summed over its blocks (hg_ctx_cluster_tree_rounds)"""
        return int(lib().hg_ctx_cluster_tree_rounds(self._h))

    # ---- the three forms of a linkage scheme on the dense matrix (average, complete), given its C function ----
    def _linkage_host(self, fn, hv, n2, ksize, ani_th):
        h = np.ascontiguousarray(hv, np.int16)
        nn = np.ascontiguousarray(n2, np.int32)
        n = h.shape[0]
        rep, cl, into, size = (np.zeros(n, np.uint32) for _ in range(4))
        level = np.zeros(n, np.float32)
        nc = C.c_size_t(0)
        self._ck(fn(self._h, _ptr(h), _ptr(nn), n, h.shape[1], ksize, C.c_float(ani_th), _ptr(rep), _ptr(cl), _ptr(into), _ptr(level),
                    _ptr(size), C.byref(nc)))
        return rep, cl, into, level, size, nc.value

    def _linkage_dev(self, fn, head, ani_th, d_rep, d_cluster, d_into, d_level, d_size):
        """head: fn's arguments in front of ani_th -- the resident sketches, or the matrix"""
        nc = C.c_size_t(0)
        self._ck(fn(self._h, *head, C.c_float(ani_th), _ptr(d_rep or 0), _ptr(d_cluster or 0), _ptr(d_into or 0), _ptr(d_level or 0),
                    _ptr(d_size or 0), C.byref(nc)))
        return nc.value

    # ---- average linkage, UPGMA (hg_cluster_average*) ---------------------------------------------
    def cluster_average(self, hv, n2, ksize=21, ani_th=95.0):
        """hg_cluster_average on host sketches: numpy (rep, cluster, into, level, size, n_clusters) -- rep[i] = the smallest
        index of i's cluster, cluster[i] = its dense id in order of rep; the dendrogram: into[b] = the name b was absorbed
        into (b itself if never), level[b] = the average ANI of that merge (0 if never), size[b] = the size of the merged
        cluster (of b's own final cluster if never)"""
        return self._linkage_host(lib().hg_cluster_average, hv, n2, ksize, ani_th)

    def cluster_average_dev(self, d_hv, d_n2, n, hv_d, d_rep, d_cluster, d_into=None, d_level=None, d_size=None, ksize=21, ani_th=95.0):
        """hg_cluster_average_dev on resident sketches (device pointers; d_into, d_level and d_size may each be None);
        returns the number of clusters"""
        return self._linkage_dev(lib().hg_cluster_average_dev, (_ptr(d_hv or 0), _ptr(d_n2 or 0), n, hv_d, ksize), ani_th,
                                 d_rep, d_cluster, d_into, d_level, d_size)

    def cluster_average_matrix_dev(self, d_ani, n, ani_th, d_rep, d_cluster, d_into=None, d_level=None, d_size=None):
        """hg_cluster_average_matrix_dev on a device-resident n x n float matrix, of which [i, j] with i < j is read
        (d_into, d_level and d_size may each be None); returns the number of clusters"""
        return self._linkage_dev(lib().hg_cluster_average_matrix_dev, (_ptr(d_ani or 0), n), ani_th, d_rep, d_cluster, d_into, d_level, d_size)

    def cluster_average_rounds(self):
        """rounds of the last average-linkage call on this ctx (hg_ctx_cluster_average_rounds)"""
        return int(lib().hg_ctx_cluster_average_rounds(self._h))

    # ---- complete linkage (hg_cluster_complete*) --------------------------------------------------
    def cluster_complete(self, hv, n2, ksize=21, ani_th=95.0):
        """hg_cluster_complete on host sketches: numpy (rep, cluster, into, level, size, n_clusters) -- rep[i] = the smallest
        index of i's cluster, cluster[i] = its dense id in order of rep; the dendrogram: into[b] = the name b was absorbed
        into (b itself if never), level[b] = the minimum ANI between the two merged clusters (0 if never), size[b] = the size of the merged
        cluster (of b's own final cluster if never)"""
        return self._linkage_host(lib().hg_cluster_complete, hv, n2, ksize, ani_th)

    def cluster_complete_dev(self, d_hv, d_n2, n, hv_d, d_rep, d_cluster, d_into=None, d_level=None, d_size=None, ksize=21, ani_th=95.0):
        """hg_cluster_complete_dev on resident sketches (device pointers; d_into, d_level and d_size may each be None);
        returns the number of clusters"""
        return self._linkage_dev(lib().hg_cluster_complete_dev, (_ptr(d_hv or 0), _ptr(d_n2 or 0), n, hv_d, ksize), ani_th,
                                 d_rep, d_cluster, d_into, d_level, d_size)

    def cluster_complete_matrix_dev(self, d_ani, n, ani_th, d_rep, d_cluster, d_into=None, d_level=None, d_size=None):
        """hg_cluster_complete_matrix_dev on a device-resident n x n float matrix, of which [i, j] with i < j is read
        (d_into, d_level and d_size may each be None); returns the number of clusters"""
        return self._linkage_dev(lib().hg_cluster_complete_matrix_dev, (_ptr(d_ani or 0), n), ani_th, d_rep, d_cluster, d_into, d_level, d_size)

    def cluster_complete_rounds(self):
        """rounds of the last complete-linkage call on this ctx (hg_ctx_cluster_complete_rounds)"""
        return int(lib().hg_ctx_cluster_complete_rounds(self._h))

    # ---- neighbour joining (hg_nj*) ---------------------------------------------------------------
    def nj(self, hv, n2, ksize=21):
        """hg_nj on host sketches: the n - 1 joins of the neighbour-joining tree as a numpy record array of NJ_JOIN_DTYPE
        (a < b the joined names, the joined node keeps a; len_a, len_b their branches in 2^-15 thousandths of an ANI percent);
        nj_newick() writes the tree"""
        h = np.ascontiguousarray(hv, np.int16)
        nn = np.ascontiguousarray(n2, np.int32)
        n = h.shape[0]
        joins = np.zeros(max(n, 1) - 1, NJ_JOIN_DTYPE)
        nj = C.c_size_t(0)
        self._ck(lib().hg_nj(self._h, _ptr(h), _ptr(nn), n, h.shape[1], ksize, _ptr(joins), C.byref(nj)))
        return joins[:nj.value]

    def nj_dev(self, d_hv, d_n2, n, hv_d, d_joins, ksize=21):
        """hg_nj_dev on resident sketches (device pointers; d_joins: n - 1 records of 24 bytes); returns the number of joins"""
        nj = C.c_size_t(0)
        self._ck(lib().hg_nj_dev(self._h, _ptr(d_hv or 0), _ptr(d_n2 or 0), n, hv_d, ksize, _ptr(d_joins or 0), C.byref(nj)))
        return nj.value

    def nj_matrix_dev(self, d_ani, n, d_joins):
        """hg_nj_matrix_dev on a device-resident n x n float matrix, of which [i, j] with i < j is read (d_joins: n - 1
        records of 24 bytes); returns the number of joins"""
        nj = C.c_size_t(0)
        self._ck(lib().hg_nj_matrix_dev(self._h, _ptr(d_ani or 0), n, _ptr(d_joins or 0), C.byref(nj)))
        return nj.value

    # ---- cluster statistics (hg_cluster_stats*) ---------------------------------------------------
    def cluster_stats(self, hv, n2, cluster, n_clusters, ksize=21, node=True, stat=True):
        """hg_cluster_stats on host sketches and a host assignment (cluster[i] < n_clusters, any labelling): numpy record
        arrays (node, stat) of NODE_STAT_DTYPE and CLUSTER_STAT_DTYPE; node=False / stat=False passes NULL and gives None"""
        h = np.ascontiguousarray(hv, np.int16)
        nn = np.ascontiguousarray(n2, np.int32)
        cl = np.ascontiguousarray(cluster, np.uint32)
        n = h.shape[0]
        nodes = np.zeros(n, NODE_STAT_DTYPE) if node else None
        stats = np.zeros(n_clusters, CLUSTER_STAT_DTYPE) if stat else None
        self._ck(lib().hg_cluster_stats(self._h, _ptr(h), _ptr(nn), n, h.shape[1], ksize, _ptr(cl), n_clusters,
                                        _ptr(nodes) if node else _ptr(0), _ptr(stats) if stat else _ptr(0)))
        return nodes, stats

    def cluster_stats_dev(self, d_hv, d_n2, n, hv_d, d_cluster, n_clusters, d_node=None, d_stat=None, ksize=21):
        """hg_cluster_stats_dev on resident sketches (device pointers; d_node or d_stat may be None, not both): n records of
        24 bytes at d_node, n_clusters records of 48 bytes at d_stat"""
        self._ck(lib().hg_cluster_stats_dev(self._h, _ptr(d_hv or 0), _ptr(d_n2 or 0), n, hv_d, ksize, _ptr(d_cluster or 0), n_clusters,
                                            _ptr(d_node or 0), _ptr(d_stat or 0)))

    def cluster_stats_matrix_dev(self, d_ani, n, d_cluster, n_clusters, d_node=None, d_stat=None):
        """hg_cluster_stats_matrix_dev on a device-resident n x n float matrix, row-major (d_node or d_stat may be None, not
        both)"""
        self._ck(lib().hg_cluster_stats_matrix_dev(self._h, _ptr(d_ani or 0), n, _ptr(d_cluster or 0), n_clusters, _ptr(d_node or 0),
                                                   _ptr(d_stat or 0)))


def shard_range(n, shard, n_shards):
    lo, hi = C.c_size_t(0), C.c_size_t(0)
    lib().hg_shard_range(n, shard, n_shards, C.byref(lo), C.byref(hi))
    return lo.value, hi.value


class Multi:
    """Several GPUs in one process (hg_multi): one hg_ctx per entry of device_ids (ids may repeat)."""

    def __init__(self, device_ids):
        ids = (C.c_int * len(device_ids))(*device_ids)
        self._h = C.c_void_p()
        st = lib().hg_multi_create(ids, len(device_ids), C.byref(self._h))
        if st != OK:
            raise HgError(st, lib().hg_last_error(None).decode())
        self.n = len(device_ids)

    def close(self):
        if self._h:
            lib().hg_multi_destroy(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _ck(self, st, allow=()):
        if st != OK and st not in allow:
            raise HgError(st, lib().hg_multi_last_error(self._h).decode())
        return st

    def ctx_handle(self, shard):
        return lib().hg_multi_ctx(self._h, shard)

    def peer_report(self):
        return lib().hg_multi_peer_report(self._h).decode()

    def set_gather(self, mode):
        """GATHER_PEER (direct hipMemcpyPeerAsync pulls) or GATHER_RCCL (ncclAllGather / grouped ncclBroadcast)."""
        self._ck(lib().hg_multi_set_gather(self._h, mode))

    def set_ani_metric(self, metric):
        """hg_multi_set_ani_metric: the ANI metric of every shard's ctx (see Context.set_ani_metric)."""
        self._ck(lib().hg_multi_set_ani_metric(self._h, metric))

    def gather_mode(self):
        return lib().hg_multi_gather_mode(self._h)

    def gather_report(self):
        return lib().hg_multi_gather_report(self._h).decode()

    def sketch_batch(self, seqs, params=None):
        return _sketch_batch_host(self._ck, lib().hg_sketch_batch_multi, self._h, seqs, params or default_params())

    def dist(self, ref_hv, ref_n2, qry_hv=None, qry_n2=None, ksize=21, symmetric=False, ani_th=85.0, cap=None):
        r = np.ascontiguousarray(ref_hv, np.int16)
        rn = np.ascontiguousarray(ref_n2, np.int32)
        q = r if qry_hv is None else np.ascontiguousarray(qry_hv, np.int16)
        qn = rn if qry_hv is None else np.ascontiguousarray(qry_n2, np.int32)
        cap = cap if cap is not None else max(1024, r.shape[0] * q.shape[0] // 8)
        while True:
            out = np.zeros(cap, ANI_HIT_DTYPE)
            n = C.c_size_t(0)
            st = lib().hg_dist_multi(self._h, _ptr(r), _ptr(rn), r.shape[0], _ptr(q), _ptr(qn), q.shape[0],
                                     r.shape[1], ksize, int(symmetric), C.c_float(ani_th), _ptr(out), cap,
                                     C.byref(n))
            if st == ERR_CAPACITY:
                cap = n.value
                continue
            self._ck(st)
            return out[: n.value].copy()

    def dist_dev(self, d_ref, d_rn, ref_rows, d_qry, d_qn, qry_rows, hv_d, ksize=21, symmetric=False, ani_th=85.0,
                 cap=1 << 20):
        """d_ref / d_rn (and d_qry / d_qn or None): per-shard device pointers (ints)."""
        arr = lambda xs: (C.c_void_p * self.n)(*[int(x) for x in xs])
        szs = lambda xs: (C.c_size_t * self.n)(*[int(x) for x in xs])
        while True:
            out = np.zeros(cap, ANI_HIT_DTYPE)
            n = C.c_size_t(0)
            st = lib().hg_dist_multi_dev(self._h, arr(d_ref), arr(d_rn), szs(ref_rows),
                                         arr(d_qry) if d_qry is not None else None,
                                         arr(d_qn) if d_qry is not None else None,
                                         szs(qry_rows) if d_qry is not None else None, hv_d, ksize, int(symmetric),
                                         C.c_float(ani_th), _ptr(out), cap, C.byref(n))
            if st == ERR_CAPACITY:
                cap = n.value
                continue
            self._ck(st)
            return out[: n.value].copy()

    def search_topk_dev(self, d_ref, d_rn, ref_rows, d_qry, d_qn, Q, hv_d, ksize=21, ani_th=85.0, k=1):
        """hg_search_topk_multi_dev: d_ref / d_rn hold each shard's reference rows, d_qry / d_qn ALL Q query rows on every
        shard (per-shard device pointers, ints); returns host (hits of shape (Q, k), counts)."""
        arr = lambda xs: (C.c_void_p * self.n)(*[int(x) for x in xs])
        szs = lambda xs: (C.c_size_t * self.n)(*[int(x) for x in xs])
        out = np.zeros((Q, k), ANI_HIT_DTYPE)
        cnt = np.zeros(Q, np.uint32)
        self._ck(lib().hg_search_topk_multi_dev(self._h, arr(d_ref), arr(d_rn), szs(ref_rows), arr(d_qry), arr(d_qn), Q, hv_d,
                                                ksize, C.c_float(ani_th), k, _ptr(out), _ptr(cnt)))
        return out, cnt

    def hamming_search(self, ref_bits, qry_bits, hv_d, max_dist, cap=1 << 20):
        r = np.ascontiguousarray(ref_bits, np.uint32)
        q = np.ascontiguousarray(qry_bits, np.uint32)
        while True:
            out = np.zeros(cap, HAM_HIT_DTYPE)
            n = C.c_size_t(0)
            st = lib().hg_hamming_search_multi(self._h, _ptr(r), r.shape[0], _ptr(q), q.shape[0], hv_d, max_dist,
                                               _ptr(out), cap, C.byref(n))
            if st == ERR_CAPACITY:
                cap = n.value
                continue
            self._ck(st)
            return out[: n.value].copy()


# ---- host-side formats (no device involved) ------------------------------------------------------
def hv_quant_bits(hv):
    hv = np.ascontiguousarray(hv, np.int16)
    return int(lib().hg_hv_quant_bits(_ptr(hv), hv.size))


def hv_pack(hv, q=None):
    hv = np.ascontiguousarray(hv, np.int16)
    q = hv_quant_bits(hv) if q is None else q
    out = np.zeros(lib().hg_hv_packed_bytes(hv.size, q), np.uint8)
    st = lib().hg_hv_pack(_ptr(hv), hv.size, q, _ptr(out))
    if st != OK:
        raise HgError(st, "hg_hv_pack")
    return q, out


def hv_unpack(packed, hv_d, q):
    packed = np.ascontiguousarray(packed, np.uint8)
    hv = np.zeros(hv_d, np.int16)
    st = lib().hg_hv_unpack(_ptr(packed), hv_d, q, _ptr(hv))
    if st != OK:
        raise HgError(st, "hg_hv_unpack")
    return hv


PAYLOAD_BITPACKER8X, PAYLOAD_NAIVE = 0, 1


def hv_pack_naive(hv, q=None):
    """the payload layout of hosts without AVX2 (src/hd.rs:158-166): (q, bytes)"""
    hv = np.ascontiguousarray(hv, np.int16)
    q = hv_quant_bits(hv) if q is None else q
    out = np.zeros(lib().hg_hv_packed_bytes_naive(hv.size, q), np.uint8)
    st = lib().hg_hv_pack_naive(_ptr(hv), hv.size, q, _ptr(out))
    if st != OK:
        raise HgError(st, "hg_hv_pack_naive")
    return q, out


def hv_unpack_naive(packed, hv_d, q):
    packed = np.ascontiguousarray(packed).view(np.uint8)
    hv = np.zeros(hv_d, np.int16)
    st = lib().hg_hv_unpack_naive(_ptr(packed), hv_d, q, _ptr(hv))
    if st != OK:
        raise HgError(st, "hg_hv_unpack_naive")
    return hv


def hv_payload_layout(hv_d, q, payload_bytes):
    return int(lib().hg_hv_payload_layout(hv_d, q, payload_bytes))


def read_sketch_file_image(path):
    """(image bytes as a numpy array, records) -- the records carry `payload_off` / `payload_bytes` instead of `hv`"""
    h = C.c_void_p()
    st = lib().hg_sketch_file_read_image(os.fsencode(path), C.byref(h))
    if st != OK:
        raise HgError(st, "hg_sketch_file_read_image(%s)" % path)
    try:
        nb = C.c_size_t(0)
        base = lib().hg_sketch_file_image(h, C.byref(nb))
        img = np.ctypeslib.as_array(C.cast(base, C.POINTER(C.c_uint8)), shape=(nb.value,)).copy() if nb.value else np.zeros(0, np.uint8)
        out = []
        for i in range(lib().hg_sketch_file_count(h)):
            r = lib().hg_sketch_file_get(h, i).contents
            assert not r.hv
            out.append(dict(ksize=r.ksize, scaled=r.scaled, canonical=bool(r.canonical), seed=r.seed,
                            hv_d=r.hv_d, hv_quant_bits=r.hv_quant_bits, hv_norm_2=r.hv_norm_2,
                            file_str=r.file_str.decode(), payload_off=int(lib().hg_sketch_file_payload_offset(h, i)),
                            payload_bytes=int(r.hv_len) * 2))
        return img, out
    finally:
        lib().hg_sketch_file_free(h)


def search_topk_merge(lists, counts, k):
    """hg_search_topk_merge: per-shard results (hits of shape (Q, k), counts) of disjoint reference sets -> one (hits, counts)"""
    ls = [np.ascontiguousarray(l, ANI_HIT_DTYPE) for l in lists]
    cs = [np.ascontiguousarray(c, np.uint32) for c in counts]
    Q = cs[0].size if cs else 0
    n = len(ls)
    lp = (C.c_void_p * max(n, 1))(*[l.ctypes.data for l in ls])
    cp = (C.c_void_p * max(n, 1))(*[c.ctypes.data for c in cs])
    out = np.zeros((Q, k), ANI_HIT_DTYPE)
    cnt = np.zeros(Q, np.uint32)
    st = lib().hg_search_topk_merge(lp, cp, n, Q, k, _ptr(out), _ptr(cnt))
    if st != OK:
        raise HgError(st, "hg_search_topk_merge")
    return out, cnt


def sort_ani_hits(hits, Q, symmetric=False):
    hits = np.ascontiguousarray(hits, ANI_HIT_DTYPE).copy()
    lib().hg_sort_ani_hits(_ptr(hits), hits.size, Q, int(symmetric))
    return hits


READ_MERGE, READ_NEEDLETAIL = 0, 1


def nj_newick(joins, names):
    """hg_nj_newick: the join list of Context.nj* (NJ_JOIN_DTYPE records, len(names) - 1 of them) and the items' names ->
    the unrooted tree in Newick form (str; names may be str or bytes).  Raises HgError(ERR_INVALID) for a list that is not a
    valid join sequence."""
    j = np.ascontiguousarray(joins, NJ_JOIN_DTYPE)
    n = len(names)
    if j.shape != (max(n, 1) - 1,):
        raise HgError(ERR_INVALID, "nj_newick: %d names take %d joins" % (n, max(n, 1) - 1))
    arr = (C.c_char_p * max(n, 1))(*[x if isinstance(x, bytes) else str(x).encode() for x in names])
    p, ln = C.c_void_p(), C.c_size_t(0)
    st = lib().hg_nj_newick(_ptr(j) if j.size else None, n, arr, C.byref(p), C.byref(ln))
    if st != OK:
        raise HgError(st, "hg_nj_newick")
    try:
        return C.string_at(p, ln.value).decode()
    finally:
        lib().hg_free(p)


def read_merge_seq(path, mode=READ_MERGE):
    p, n, cap = C.c_void_p(), C.c_size_t(0), C.c_size_t(0)
    st = lib().hg_read_fastx_into(os.fsencode(path), mode, C.byref(p), C.byref(cap), C.byref(n))
    if st != OK:
        lib().hg_free(p)
        raise HgError(st, "hg_read_fastx_into(%s)" % path)
    try:
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(n.value,)).copy() if n.value \
            else np.zeros(0, np.uint8)
    finally:
        lib().hg_free(p)


def pack2s(seq, norm_mode=0, cap=None):
    """hg_pack2s: the sparse link form (2-bit codes + a table of the not-a-base runs), or None if the table does not fit
    `cap` bytes (default: the size of the hg_pack2 blob -- beyond that the bitmap form is the smaller one)."""
    a = np.ascontiguousarray(seq, np.uint8)
    n = a.size
    cap = lib().hg_pack2_size(n) if cap is None else cap
    out = np.empty(max(cap, 16), np.uint8)
    size = C.c_size_t(0)
    st = lib().hg_pack2s(_ptr(a), n, norm_mode, _ptr(out), out.size, C.byref(size))
    if st == ERR_CAPACITY:
        return None
    if st != OK:
        raise HgError(st, "hg_pack2s")
    return out[:size.value]


def pack2(seq, norm_mode=0, in_place=False):
    """hg_pack2: uint8 blob of hg_pack2_size(len(seq)) bytes (2-bit codes + not-a-base bits)."""
    a = np.ascontiguousarray(seq, np.uint8)
    n = a.size
    size = lib().hg_pack2_size(n)
    if in_place:
        buf = np.zeros(max(n, size), np.uint8)
        buf[:n] = a
        st = lib().hg_pack2(_ptr(buf), n, norm_mode, _ptr(buf))
        out = buf[:size]
    else:
        out = np.empty(size, np.uint8)
        st = lib().hg_pack2(_ptr(a), n, norm_mode, _ptr(out))
    if st != OK:
        raise HgError(st, "hg_pack2")
    return out


class PinnedReader:
    """Page-locked read buffers (hg_read_fastx_pinned): read(path) returns a uint8 view that stays valid until
    the next read into the same slot or close(); what the CLI's reader threads use to feed hg_sketch_batch."""

    def __init__(self, slots=1):
        self._p = [C.c_void_p() for _ in range(slots)]
        self._cap = [C.c_size_t(0) for _ in range(slots)]

    def read(self, path, slot=0, mode=READ_MERGE):
        n = C.c_size_t(0)
        st = lib().hg_read_fastx_pinned(os.fsencode(path), mode, C.byref(self._p[slot]), C.byref(self._cap[slot]), C.byref(n))
        if st != OK:
            raise HgError(st, "hg_read_fastx_pinned(%s)" % path)
        if not n.value:
            return np.zeros(0, np.uint8)
        return np.ctypeslib.as_array(C.cast(self._p[slot], C.POINTER(C.c_uint8)), shape=(n.value,))

    def close(self):
        for p in self._p:
            if p:
                lib().hg_pinned_free(p)
                p.value = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class SketchStream:
    """Continuous host-fed sketching (hg_sketch_stream_*): push(seq, tag) from any thread, pop() -> (tag, hv, norm2,
    nhash) in completion order (None once finish() was called and everything has been popped).  The arrays pushed
    are kept alive until their result is popped."""

    def __init__(self, device_ids=(0,), params=None):
        self.params = params or default_params()
        ids = (C.c_int * len(device_ids))(*device_ids)
        self._h = C.c_void_p()
        st = lib().hg_sketch_stream_open(ids, len(device_ids), C.byref(self.params), C.byref(self._h))
        if st != OK:
            raise HgError(st, "hg_sketch_stream_open: " + lib().hg_last_error(None).decode())
        self._keep = {}      # internal id -> (user tag, the array the device may still read)
        self._next = 0
        self._ready = []     # results popped on the pusher's behalf while the stream was full
        self._lock = threading.Lock()

    def _check(self, st, what):
        if st != OK:
            raise HgError(st, what + ": " + lib().hg_sketch_stream_last_error(self._h).decode())

    def _push(self, a, n_bps, tag, packed):
        # The C push blocks once max_pending results are outstanding; a caller that pushes everything before it pops
        # (the natural single-threaded use) would wait for ever.  So: never block here -- when the stream is full, take
        # one finished result out and hand it over on a later pop().  Arrays are kept by an internal id, not by the
        # user's tag (a reused tag must not drop the keep-alive of an array the device may still read).
        with self._lock:
            iid = self._next
            self._next += 1
            self._keep[iid] = (tag, a)
        try:
            while True:
                st = lib().hg_sketch_stream_try_push(self._h, _ptr(a), n_bps, iid, int(packed))
                if st != ERR_CAPACITY:
                    break
                r = self._pop_c()
                if r is not None:
                    with self._lock:
                        self._ready.append(r)
        except BaseException:  # a stream error surfaced by the pop: the genome was never queued, drop its keep-alive
            with self._lock:
                self._keep.pop(iid, None)
            raise
        if st != OK:
            with self._lock:
                self._keep.pop(iid, None)
        self._check(st, "hg_sketch_stream_try_push")

    def push(self, seq, tag):
        a = np.ascontiguousarray(seq, np.uint8)
        self._push(a, a.size, tag, 0)

    def push_packed(self, blob, n_bps, tag):
        a = np.ascontiguousarray(blob, np.uint8)
        assert a.size >= lib().hg_pack2_size(n_bps)
        self._push(a, n_bps, tag, 1)

    def push_packed_sparse(self, blob, n_bps, tag):
        """a hg_pack2s blob (pack2s()): codes + run table.  The buffer must hold the whole blob (checked here: the
        non-blocking C entry point takes the caller's word for the size; the library validates the table's contents)."""
        a = np.ascontiguousarray(blob, np.uint8)
        tab = (((n_bps + 3) // 4) + 15) & ~15
        if n_bps and (a.size < tab + 8 or a.size < lib().hg_pack2s_size(n_bps, int(a[tab: tab + 4].view("<u4")[0]))):
            raise HgError(ERR_INVALID, "push_packed_sparse: the buffer is shorter than the blob it claims to hold")
        self._push(a, n_bps, tag, 2)

    def finish(self):
        self._check(lib().hg_sketch_stream_finish(self._h), "hg_sketch_stream_finish")

    def _pop_c(self):
        iid, n2, nh, got = C.c_uint64(), C.c_int32(), C.c_uint32(), C.c_int()
        hv = np.empty(self.params.hv_d, np.int16)
        self._check(lib().hg_sketch_stream_pop(self._h, C.byref(iid), _ptr(hv), C.byref(n2), C.byref(nh), C.byref(got)),
                    "hg_sketch_stream_pop")
        if not got.value:
            return None
        with self._lock:
            tag, _ = self._keep.pop(iid.value)
        return tag, hv, n2.value, nh.value

    def pop(self):
        with self._lock:
            if self._ready:
                return self._ready.pop(0)
        return self._pop_c()

    def stats(self, engine=0):
        out = (C.c_double * 6)()
        self._check(lib().hg_sketch_stream_stats(self._h, engine, out), "hg_sketch_stream_stats")
        return dict(zip(("uploader_idle_s", "uploader_no_chunk_s", "uploader_copy_s", "compute_idle_s", "compute_busy_s",
                         "chunks"), out))

    def close(self):
        if self._h:
            lib().hg_sketch_stream_close(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


def sketch_plan_describe(offsets, lens, ksize=21, scaled=1500):
    """hg_sketch_plan_describe: (dict of counts, group_first array or None) -- host arithmetic, needs no GPU"""
    off = np.ascontiguousarray(offsets, np.uint64)
    ln = np.ascontiguousarray(lens, np.uint64)
    counts = (C.c_uint64 * 6)()
    st = lib().hg_sketch_plan_describe(_ptr(off), _ptr(ln), off.size, ksize, scaled, counts, None, 0)
    if st != OK:
        raise HgError(st, "hg_sketch_plan_describe")
    d = dict(zip(("items", "workgroups", "hit_slots", "max_cap", "max_expect", "item_tiles"), (int(x) for x in counts)))
    gf = None
    if ksize <= 32 and d["items"]:
        gf = np.zeros(d["workgroups"] + 1, np.uint32)
        st = lib().hg_sketch_plan_describe(_ptr(off), _ptr(ln), off.size, ksize, scaled, counts, _ptr(gf), gf.size)
        if st != OK:
            raise HgError(st, "hg_sketch_plan_describe")
    return d, gf


def write_sketch_file(path, records):
    """records: dicts with ksize, scaled, canonical, seed, hv_d, hv_quant_bits, hv_norm_2, file_str, hv."""
    arr = (FileSketch * max(len(records), 1))()
    keep = []
    for i, r in enumerate(records):
        hv = np.ascontiguousarray(r["hv"], np.int16)
        name = r["file_str"].encode()
        keep += [hv, name]
        arr[i] = FileSketch(r["ksize"], int(bool(r["canonical"])), r["hv_quant_bits"], 0, r["hv_norm_2"],
                            r["scaled"], r["seed"], r["hv_d"], name,
                            hv.ctypes.data_as(C.POINTER(C.c_int16)), hv.size)
    st = lib().hg_sketch_file_write(os.fsencode(path), arr, len(records))
    if st != OK:
        raise HgError(st, "hg_sketch_file_write(%s)" % path)


def read_sketch_file(path):
    h = C.c_void_p()
    st = lib().hg_sketch_file_read(os.fsencode(path), C.byref(h))
    if st != OK:
        raise HgError(st, "hg_sketch_file_read(%s)" % path)
    try:
        out = []
        for i in range(lib().hg_sketch_file_count(h)):
            r = lib().hg_sketch_file_get(h, i).contents
            hv = np.ctypeslib.as_array(r.hv, shape=(r.hv_len,)).copy() if r.hv_len else np.zeros(0, np.int16)
            out.append(dict(ksize=r.ksize, scaled=r.scaled, canonical=bool(r.canonical), seed=r.seed,
                            hv_d=r.hv_d, hv_quant_bits=r.hv_quant_bits, hv_norm_2=r.hv_norm_2,
                            file_str=r.file_str.decode(), hv=hv))
        return out
    finally:
        lib().hg_sketch_file_free(h)
