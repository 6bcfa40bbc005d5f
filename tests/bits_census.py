"""One row per compiled kernel of libhypergen_hip.so that works on packed bits -- sign bits of hypervectors, bit-packed sketch
payloads, 2-bit bases, the synthetic genomes' code words -- and how an input reaches it.  Their names match neither
kernel_census.py's families nor set_encode_census.py's, so they have a table of their own.

test_bits_census.py (CPU) checks that the names here are exactly the instantiations `nm -C` finds in the built library: a
kernel added without a row, or a row whose kernel is gone, fails there.  test_gpu_bits_census.py (GPU) runs every row at one
small input and every kernel at the shapes where a bit position, a word boundary or an alignment decides.

A row's name is spelled as hg_ctx_last_kernel and rocprofv3 spell it.  Its route:
* entry: "binarize" (hg_hv_binarize_dev), "hamming" (hg_hamming_search_dev; the popcount rows also through
  hg_hamming_full_dev), "unpack" (hg_hv_unpack_batch_dev), "pack2" (hg_pack2_batch_dev), "unpack2" (hg_unpack2_dev), "stream"
  (hg_sketch_stream_*) or "synth" (hg_synth_genomes_dev);
* debug: the hg_ctx_set_debug keys the call runs under (ham_path); none: the library chooses;
* inputs: what the input has to be for the kernel to run -- the number of query rows that selects a popcount tile, the
  in-kernel routes of the payload decoder, the forms of a stream's chunk;
* unreachable: None, or why no input reaches the kernel (printed by the CPU test).
"""
from collections import namedtuple

Row = namedtuple("Row", "name entry debug inputs unreachable")

# hg_hv_unpack_kernel decides per payload (workgroup): staged through LDS or direct, and which layout it decodes
UNPACK_ROUTES = tuple((stage, layout) for stage in ("staged", "direct") for layout in ("bitpacker8x", "naive"))

HAMMING_ROWS = [
    # JN query columns per lane: the tile is 128 references x 16 JN queries (ham_launch: Q <= 16, Q <= 32, more);
    # ctx.last_kernel("dist") names the row
    Row("hamming_kernel<1>", "hamming", {"ham_path": "popc"}, {"Q": 16}, None),
    Row("hamming_kernel<2>", "hamming", {"ham_path": "popc"}, {"Q": 32}, None),
    Row("hamming_kernel<8>", "hamming", {"ham_path": "popc"}, {"Q": 129}, None),
]
EXPAND_ROWS = [
    # bits -> the matrix pipe's operands: +-1 bytes ("mfma", hv_d % 128 == 0) or e2m1 nibbles ("fp4"); last_kernel names
    # the GEMM they feed, ctx.last_hamming_path() the operand form
    Row("expand_bits_kernel", "hamming", {"ham_path": "mfma"}, {"Q": 129}, None),
    Row("expand_bits_fp4_kernel", "hamming", {"ham_path": "fp4"}, {"Q": 129}, None),
]
OTHER_ROWS = [
    Row("binarize_kernel", "binarize", {}, "hv", None),
    Row("hg_hv_unpack_kernel", "unpack", {}, UNPACK_ROUTES, None),
    Row("pack2_kernel", "pack2", {}, "seq", None),
    Row("unpack2_one_kernel", "unpack2", {}, "blob", None),
    # a chunk that holds ASCII and packed genomes: the blobs are expanded into the sequence buffer
    Row("unpack2_kernel", "stream", {}, ("ascii", "packed"), None),
    # a chunk with a genome that came as codes + run table: its bitmap is rebuilt on the device
    Row("expand_runs_kernel", "stream", {}, ("sparse",), None),
    Row("synth_kernel", "synth", {}, "counter", None),
]
ROWS = HAMMING_ROWS + EXPAND_ROWS + OTHER_ROWS
