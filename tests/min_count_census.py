"""One row per compiled min_count_* kernel of libhypergen_hip.so -- the set stage's second family, launched in place of
sort_unique_* / bucket_sort_kernel when hg_sketch_params.min_count > 1 -- and how an input reaches it.

test_min_count_census.py (CPU) checks the names against what `nm -C` finds in the built library; test_gpu_min_count.py (GPU) runs
every row: ctx.last_kernel("sort") must name the kernel, and the result must equal min_count_ref's.

A row's route, as in set_encode_census.py: entry ("sketch_batch_dev": the sync-free step; "sync": the synchronous path),
the hg_ctx_set_debug keys the call runs under, the input classes of test_gpu_min_count.py that land on the row, and
`twin`: the kernel of the first family whose body (a device function with the MINC flag) it shares.
"""
from collections import namedtuple

Row = namedtuple("Row", "name twin entry debug inputs unreachable")

ROWS = [
    Row("min_count_wave_kernel", "sort_unique_wave_kernel", "sketch_batch_dev", {}, ("tiny",), None),
    Row("min_count_kernel<true>", "sort_unique_kernel<true>", "sketch_batch_dev", {}, ("lds", "bucket16", "edges"), None),
    Row("min_count_rest_kernel", "sort_unique_rest_kernel", "sketch_batch_dev", {}, ("tiny", "outgrow"), None),
    Row("min_count_bucket_kernel", "bucket_sort_kernel", "sync", {}, ("large", "table", "lookahead", "reads"), None),
    Row("min_count_kernel<false>", "sort_unique_kernel<false>", "sync", {"sort_test_buckets": "2"}, ("inplace",), None),
]

ENTRIES = ("sketch_batch_dev", "sync")


def sort_launches(launches, m):
    """the launch list of set_encode_census.dispatch (min_count <= 1) as the min_count family reports it for m > 1"""
    if m <= 1:
        return list(launches)
    twin = {r.twin: r.name for r in ROWS}
    return [twin.get(k, k) for k in launches]
