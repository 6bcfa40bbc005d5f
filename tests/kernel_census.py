"""One row per compiled dist and k-mer kernel instantiation of libhypergen_hip.so, and how an input reaches it.

test_kernel_census.py (CPU) checks that the names here are exactly the `dist_*kernel` and `kmer_sample_*<...>` instantiations
`nm -C` finds in the built library: a kernel added without a row, or a row whose kernel is gone, fails there.
test_gpu_kernel_census.py (GPU) runs every row and checks ctx.last_kernel() and the result against an exact reference.

A row's name is spelled as hg_ctx_last_kernel and rocprofv3 spell it.  Its route:
* entry: "dist" (thresholded hit list, hg_dist), "dist_full" (the full matrix, hg_dist_full), "hamming" (hg_hamming_search_dev)
  or "kmer" (hg_kmer_hash_sample);
* debug: the hg_ctx_set_debug keys the call runs under (dist_path, dist_tile, ham_path, hostfed); none: the library chooses;
* metric: "mash" (dist_mfma_kernel / the metric-generic kernels) or "ctm" (the containment metrics: HG_ANI_CONTAINMENT and
  HG_ANI_MAX_CONTAINMENT share one instantiation);
* inputs: the input class (see test_gpu_kernel_census.py): "sketch" (whole-K sketches), "win" (sketches that need accumulation
  windows: verdicts 1, 2 and the non-speculative rerun), "skinny_q" / "skinny_r" (a handful of rows on one side), "wide"
  (values beyond f16's exact integers), "bits" (bit-packed hypervectors), "seq" (a sequence);
* unreachable: None, or why no input reaches the kernel (printed by the CPU test).
"""
from collections import namedtuple

Row = namedtuple("Row", "name entry debug metric inputs unreachable")


def _b(x):
    return "true" if x else "false"


def mfma_name(chunked, full, big, glds, nt, i8=False, ham=False, fp4=False, cen=False, ctm=False):
    """tile_kernel()'s spelling (hg_dist_kernels.hip)"""
    args = [_b(chunked), _b(full), _b(big), _b(glds), str(nt), _b(i8)] + ([] if ctm else [_b(ham), _b(fp4)]) + [_b(cen)]
    return ("dist_mfma_ctm_kernel<" if ctm else "dist_mfma_kernel<") + ", ".join(args) + ">"


def _dist_rows():
    rows = []
    for ctm in (False, True):
        m = "ctm" if ctm else "mash"

        def add(name, entry, debug, inputs):
            rows.append(Row(name, entry, debug, m, inputs, None))

        # the raw-value chain (f16 copies of the values): 128 x 128 full matrices and hit lists, 256 x 256 / 320 hit lists,
        # and the same with accumulation windows (NT = 3 on big tiles)
        add(mfma_name(False, True, False, False, 4, ctm=ctm), "dist_full", {"dist_path": "f16"}, "sketch")
        add(mfma_name(False, False, False, False, 4, ctm=ctm), "dist", {"dist_path": "f16", "dist_tile": "small"}, "sketch")
        add(mfma_name(False, False, True, True, 4, ctm=ctm), "dist", {"dist_path": "f16", "dist_tile": "big"}, "sketch")
        add(mfma_name(False, False, True, True, 5, ctm=ctm), "dist", {"dist_path": "f16", "dist_tile": "wide"}, "sketch")
        add(mfma_name(True, True, False, False, 4, ctm=ctm), "dist_full", {"dist_path": "f16"}, "win")
        add(mfma_name(True, False, False, False, 4, ctm=ctm), "dist", {"dist_path": "f16", "dist_tile": "small"}, "win")
        add(mfma_name(True, False, True, True, 3, ctm=ctm), "dist", {"dist_path": "f16", "dist_tile": "big"}, "win")
        # centred f16 operands
        add(mfma_name(False, False, True, True, 4, cen=True, ctm=ctm), "dist", {"dist_path": "cen", "dist_tile": "big"}, "sketch")
        add(mfma_name(False, False, True, True, 5, cen=True, ctm=ctm), "dist", {"dist_path": "cen", "dist_tile": "wide"}, "sketch")
        # byte operands (the containment metrics: 256 x 256 tiles only, whatever dist_tile says)
        add(mfma_name(False, False, True, True, 4, i8=True, ctm=ctm), "dist", {"dist_path": "i8", "dist_tile": "big"}, "sketch")
        if not ctm:
            add(mfma_name(False, False, True, True, 5, i8=True), "dist", {"dist_path": "i8", "dist_tile": "wide"}, "sketch")
    # the bit-packed Hamming search on the matrix pipe: +-1 bytes ("mfma") or e2m1 nibbles ("fp4")
    for fp4 in (False, True):
        for nt, tile in ((4, "big"), (5, "wide")):
            rows.append(Row(mfma_name(False, False, True, True, nt, i8=True, ham=True, fp4=fp4), "hamming",
                            {"ham_path": "fp4" if fp4 else "mfma", "dist_tile": tile}, "mash", "bits", None))
    # a handful of rows on one side (no hooks), values beyond f16 (the integer kernel)
    rows.append(Row("dist_skinny_kernel<false>", "dist", {}, "any", "skinny_q", None))
    rows.append(Row("dist_skinny_kernel<true>", "dist", {}, "any", "skinny_r", None))
    rows.append(Row("dist_int_kernel", "dist", {}, "any", "wide", None))
    return rows


KMER_LONG_KS = (65, 100, 255)  # kmer_sample_long<0, ...>: k as a run-time value


def _kmer_rows():
    rows = []
    for k in range(1, 33):
        for canon in (False, True):
            for packed in (False, True):
                rows.append(Row("kmer_sample_shared<%d, %s, %s>" % (k, _b(canon), _b(packed)), "kmer",
                                {"hostfed": "packed" if packed else "ascii"}, None, (k, canon), None))
    for k in list(range(33, 65)) + [0]:
        for packed in (False, True):
            # (canonical is a run-time argument here: both values run against the same instantiation)
            rows.append(Row("kmer_sample_long<%d, %s>" % (k, _b(packed)), "kmer", {"hostfed": "packed" if packed else "ascii"},
                            None, (k,) if k else KMER_LONG_KS, None))
    return rows


DIST_ROWS = _dist_rows()
KMER_ROWS = _kmer_rows()
ROWS = DIST_ROWS + KMER_ROWS


def kmer_kernel_name(k, canonical, packed):
    """hg_kmer_kernel_name (hg_kmer_kernels.hip)"""
    if k > 32:
        return "kmer_sample_long<%d, %s>" % (k if k <= 64 else 0, _b(packed))
    return "kmer_sample_shared<%d, %s, %s>" % (k, _b(canonical), _b(packed))
