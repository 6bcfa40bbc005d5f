"""One row per compiled set-stage (sort / unique) and encode-stage kernel of libhypergen_hip.so, how an input reaches it, and a
host mirror of the dispatch that sends each genome of a batch to one of them.

test_set_encode_census.py (CPU) checks that the names here are exactly the `sort_unique*`, `bucket_*_kernel`, `encode*_kernel`
and `sketch_finish_kernel` instantiations `nm -C` finds in the built library, and pins the mirror against
hg_sketch_plan_describe.  test_gpu_set_encode_census.py (GPU) runs every row: ctx.last_kernel("sort" / "encode") must equal the
launch list the mirror predicts, the mirror must send the planted genome to the row, and the result must equal the oracle's
bit for bit.

A row's route:
* entry: "hv_encode" (hg_hv_encode), "sketch_batch_dev" (the sync-free step), "sync" (hg_sketch_batch_dev under
  sketch_path = sync, or a sync-free step run again through it);
* debug: the hg_ctx_set_debug keys the call runs under;
* inputs: the input classes of test_gpu_set_encode_census.py that plant a genome on the row;
* unreachable: None, or why no input reaches the kernel (printed by the CPU test).
"""
from collections import namedtuple

Row = namedtuple("Row", "name entry debug inputs unreachable")

ROWS = [
    # ---- set stage ----
    Row("sort_unique_wave_kernel", "sketch_batch_dev", {}, ("tiny", "double"), None),
    Row("sort_unique_kernel<true>", "sketch_batch_dev", {}, ("lds", "bucket16", "seen_redo"), None),
    Row("sort_unique_rest_kernel", "sketch_batch_dev", {}, ("double", "outgrow"), None),
    Row("sort_unique_kernel<false>", "sync", {"sort_test_buckets": "2"}, ("inplace",), None),
    Row("bucket_count_kernel", "sync", {}, ("large", "global_buckets"), None),
    Row("bucket_scan_kernel", "sync", {}, ("large",), None),
    Row("bucket_scatter_kernel", "sync", {}, ("large", "global_buckets"), None),
    Row("bucket_sort_kernel", "sync", {}, ("large", "inplace"), None),
    Row("bucket_copy_kernel", "sync", {}, ("large",), None),
    Row("sketch_finish_kernel", "sketch_batch_dev", {}, ("tiny",), None),
    # ---- encode stage ----
    Row("encode_wave_kernel", "hv_encode", {}, ("planes", "wave_max"), None),
    Row("encode_kernel<false>", "hv_encode", {}, ("planes", "saturated", "wave_max"), None),
    Row("encode_kernel<true>", "sync", {}, ("slab",), None),
    Row("encode_finalize_kernel", "sync", {}, ("slab",), None),
]

ENTRIES = ("hv_encode", "sketch_batch_dev", "sync")

# ---- the dispatch, on the host ----------------------------------------------------------------------------------------
# Kernel constants (hg_sort_kernels.hip / hg_encode_kernels.hip / hg_internal.h).  The batch quantities -- every genome's hit region, the largest
# region, the largest expected count -- come from hg_sketch_plan_describe.
LDS_MAX_KEYS = 8192      # HG_SORT_LDS_MAX_KEYS
SORT_WG = 512
BUCKET_LIMIT = 16        # SORT_BUCKET_LIMIT
WAVE_MAX_BIG = 16368     # HG_ENC_WAVE_MAX
WAVE_BATCH = 8192        # genomes from which the wave kernel takes sets up to WAVE_MAX_BIG
SLAB = 32768             # HG_ENC_SLAB
BK_PRIV_MAX = 2048       # buckets a genome counts in LDS
M64 = (1 << 64) - 1


def pow2_at_least(v):
    p = 1
    while p < v:
        p <<= 1
    return p


def lds_keys(cap):
    """hg_sort_lds_keys"""
    return min(pow2_at_least(max(cap, 1)), LDS_MAX_KEYS)


def offsets_for(lens):
    import numpy as np
    return np.concatenate([[0], np.cumsum((np.asarray(lens, np.uint64) + 15) // 16 * 16)[:-1]]).astype(np.uint64)


def describe(hg, lens, k, scaled):
    """(largest hit region, largest expected count, every genome's hit region) of a batch, from hg_sketch_plan_describe"""
    d, _ = hg.sketch_plan_describe(offsets_for(lens), lens, k, scaled)
    caps = []
    memo = {}
    for L in lens:
        L = int(L)
        if L not in memo:
            memo[L] = hg.sketch_plan_describe(offsets_for([L]), [L], k, scaled)[0]["max_cap"]
        caps.append(memo[L])
    return d["max_cap"], d["max_expect"], caps


def counting_sort_over(hashes, n, keys, threshold):
    """True when the LDS counting sort of these n raw keys (sorted by a launch holding `keys` keys) puts more than
    BUCKET_LIMIT keys into one bucket -- the genome falls back to the bitonic network"""
    n2 = pow2_at_least(n)
    cnt = {}
    for h in hashes:
        b = sort_bucket(h, n2, keys, threshold)
        cnt[b] = cnt.get(b, 0) + 1
    return max(cnt.values()) > BUCKET_LIMIT


def lds_branch(n, keys, threshold, hashes):
    """what sort_unique_one<true> does with n raw keys in a launch of `keys` LDS keys"""
    if n <= 1:
        return "trivial"
    if n <= 64:
        return "wave"
    if n >= SORT_WG and keys <= LDS_MAX_KEYS and threshold:
        if hashes is None:
            return "counting"
        return "counting>bitonic" if counting_sort_over(hashes, n, keys, threshold) else "counting"
    return "bitonic"


def encode_branch(d, n_genomes, hv_d, layout, aligned, max_hashes, split_genome):
    """(kernel, detail) that writes a genome's row, plus the split kernels when the genome is in the split plan"""
    wave_max = WAVE_MAX_BIG if n_genomes >= WAVE_BATCH else 256
    if d <= wave_max:
        vec_ok = hv_d % 8 == 0 and aligned
        if vec_ok and d < 16 and layout == 1:
            detail = "lds4"
        elif layout == 1:
            detail = "p4" if d < 16 else "p6" if d < 64 else "p8" if d < 256 else "p14"
        else:
            detail = "scalar14"
        detail += "" if detail == "lds4" else ("/vec" if vec_ok else "/plain")
        if hv_d % 64:
            detail += "/tail"
        kern = "encode_wave_kernel"
    elif split_genome and d > SLAB:
        kern, detail = "encode_kernel<true>", "slabs"
    else:
        assert max_hashes > wave_max
        kern, detail = "encode_kernel<false>", "block"
    if split_genome:
        return kern, detail + "+finalize"
    return kern, detail


Dispatch = namedtuple("Dispatch", "path sort encode sort_branch encode_branch keys")


def sort_bucket(h, n2, keys, threshold):
    """the counting-sort bucket of key h in a set of n2 (a power of two) keys sorted by a launch of `keys` LDS keys"""
    mul = min(((keys << 64) + threshold - 1) // threshold, M64)
    b = ((int(h) * mul) >> 64 & 0xFFFFFFFF) >> (keys.bit_length() - n2.bit_length())
    return min(b, n2 - 1)


def dispatch(hg, entry, lens, raw, distinct, k, scaled, hv_d, layout, aligned=True, debug=None, seen=0, hashes=None):
    """The launch lists ctx.last_kernel("sort") / ("encode") report after the call, and the branch that handles every genome.

    entry: "hv_encode" (lens / k / scaled unused, one genome of distinct[0] hashes), "sketch_batch_dev" (the step; it may turn
    synchronous, or be run again synchronously when a genome outgrows the one-workgroup sort -- the lists are then that run's).
    raw / distinct: per-genome sampled hit counts with and without repeats.  seen: the largest raw count of the last synchronous
    run of the same batch geometry on the ctx (0: none).  hashes: per-genome raw hash lists, for the counting-sort bucket check."""
    debug = debug or {}
    n = len(distinct)
    if entry == "hv_encode":
        d = int(distinct[0])
        enc = ["encode_wave_kernel"] + (["encode_kernel<false>"] if d > 256 else [])
        return Dispatch("hv_encode", None, enc, None, [encode_branch(d, 1, hv_d, layout, True, d, False)], None)
    assert entry == "sketch_batch_dev"
    max_cap, max_expect, caps = describe(hg, lens, k, scaled)
    assert all(int(r) <= c for r, c in zip(raw, caps)), "a genome outgrows its hit region: not mirrored"
    threshold = M64 // scaled
    hs = lambda g: None if hashes is None else hashes[g]  # noqa: E731
    sync_free = (debug.get("sketch_path") != "sync" and not int(debug.get("sort_test_buckets", 0)) and n > 0
                 and max_expect + max_expect // 8 + 64 <= LDS_MAX_KEYS)
    if sync_free and all(int(r) <= LDS_MAX_KEYS for r in raw):
        base = seen or max_expect
        margin = 24 if base + base // 8 + 24 <= 64 else 64
        keys = lds_keys(min(max_cap, base + base // 8 + margin))
        keys2 = lds_keys(max_cap)
        sort = ["sort_unique_wave_kernel" if keys <= 64 else "sort_unique_kernel<true>"]
        if keys < keys2:
            sort.append("sort_unique_rest_kernel")
        sb = []
        for g in range(n):
            r = int(raw[g])
            if keys <= 64:
                if r <= 64:
                    b = ("sort_unique_wave_kernel", "trivial" if r <= 1 else "wave")
                    if r > keys and keys < keys2:  # the rest launch sorts it again
                        b = ("sort_unique_wave_kernel+sort_unique_rest_kernel", "wave+" + lds_branch(r, keys2, threshold, hs(g)))
                else:
                    b = ("sort_unique_rest_kernel", lds_branch(r, keys2, threshold, hs(g)))
            elif r <= keys:
                b = ("sort_unique_kernel<true>", lds_branch(r, keys, threshold, hs(g)))
            else:
                b = ("sort_unique_rest_kernel", lds_branch(r, keys2, threshold, hs(g)))
            sb.append(b)
        max_hashes = min(max_cap, LDS_MAX_KEYS)
        wave_max = WAVE_MAX_BIG if n >= WAVE_BATCH else 256
        enc = ["encode_wave_kernel"] + (["encode_kernel<false>"] if max_hashes > wave_max else []) + ["sketch_finish_kernel"]
        eb = [encode_branch(int(distinct[g]), n, hv_d, layout, aligned, max_hashes, False) for g in range(n)]
        return Dispatch("sync_free", sort, enc, sb, eb, (keys, keys2))
    # the synchronous path (hg_sketch_rare.hip); a step run again there reuses the step's plan, whose last-seen count is 0
    sort_cap = max_cap
    if seen:
        sort_cap = min(sort_cap, seen + seen // 8 + 16)
    keys, keys_all = lds_keys(sort_cap), lds_keys(max_cap)
    sort = ["sort_unique_wave_kernel" if keys <= 64 else "sort_unique_kernel<true>"]
    sb = [None] * n
    todo = []
    for g in range(n):
        r = int(raw[g])
        if r <= keys:
            sb[g] = ("sort_unique_wave_kernel", "trivial" if r <= 1 else "wave") if keys <= 64 else \
                ("sort_unique_kernel<true>", lds_branch(r, keys, threshold, hs(g)))
        elif r <= LDS_MAX_KEYS:
            todo.append(g)
            sb[g] = ("sort_unique_kernel<true>", "todo/" + lds_branch(r, keys_all, threshold, hs(g)))
            if keys <= 64 and r <= 64:  # the wave kernel sorted it already
                sb[g] = ("sort_unique_wave_kernel+sort_unique_kernel<true>", "wave+todo/" + sb[g][1][5:])
    if keys < keys_all and todo:
        sort.append("sort_unique_kernel<true>")
    buckets = int(debug.get("sort_test_buckets", 0))
    jobs, inplace = [], []
    cap_keys = 4 * 1024
    for g in range(n):
        r = int(raw[g])
        if r <= LDS_MAX_KEYS:
            continue
        P = 2
        while P < 16384 and P * 1024 < r:
            P <<= 1
        if P > BK_PRIV_MAX and r <= BK_PRIV_MAX * 4096:
            P = BK_PRIV_MAX
        if buckets:
            P = max(2, buckets)
        elif P * (LDS_MAX_KEYS // 2) < r:
            inplace.append(g)
            continue
        cap_keys = max(cap_keys, 4 * (-(-r // P)))
        jobs.append((g, P))
    launch_cap = SORT_WG
    while launch_cap < (LDS_MAX_KEYS if buckets else cap_keys) and launch_cap < LDS_MAX_KEYS:
        launch_cap <<= 1
    for g, P in jobs:
        where = "bucket_lds" if P <= BK_PRIV_MAX else "bucket_global"
        fail = False
        if hs(g) is not None:
            mul = min(((P << 64) + threshold - 1) // threshold, M64)
            per, counts = {}, {}
            for h in hs(g):
                b = min((int(h) * mul) >> 64, P - 1)
                per.setdefault(b, set()).add(int(h))
                counts[b] = counts.get(b, 0) + 1
            over = [b for b in counts if counts[b] > launch_cap]
            fail = any(len(per[b]) > launch_cap // 4 * 3 for b in over)
            if over and not fail:
                where += "/hashset"
        if fail:
            inplace.append(g)
            sb[g] = ("sort_unique_kernel<false>", where + "/gave_up")
        else:
            sb[g] = ("bucket_sort_kernel", where)
    for g in inplace:
        if sb[g] is None:
            sb[g] = ("sort_unique_kernel<false>", "inplace")
    if jobs:
        sort += ["bucket_count_kernel", "bucket_scan_kernel", "bucket_scatter_kernel", "bucket_sort_kernel",
                 "bucket_scan_kernel", "bucket_copy_kernel"]
    if inplace:
        sort.append("sort_unique_kernel<false>")
    big = [g for g in range(n) if int(raw[g]) > SLAB]
    split = 0 < len(big) < 65536
    max_hits = max([int(r) for r in raw] or [0])
    wave_max = WAVE_MAX_BIG if n >= WAVE_BATCH else 256
    enc = ["encode_wave_kernel"] + (["encode_kernel<false>"] if max_hits > wave_max else [])
    if split:
        enc += ["encode_kernel<true>", "encode_finalize_kernel"]
    eb = [encode_branch(int(distinct[g]), n, hv_d, layout, aligned, max_hits, split and g in big) for g in range(n)]
    return Dispatch("sync", sort, enc, sb, eb, (keys, keys_all))
