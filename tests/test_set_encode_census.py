"""The census of set- and encode-stage kernels (tests/set_encode_census.py) against the built library, and its host mirror of the
dispatch against hg_sketch_plan_describe -- on the CPU.  (test_gpu_set_encode_census.py runs the rows.)"""
import re
import subprocess

import numpy as np
import pytest

import set_encode_census as sc

FAMILIES = re.compile(r"::(sort_unique[a-z_]*(?:<[^>()]*>)?|bucket_[a-z]+_kernel|encode[a-z_]*_kernel(?:<[^>()]*>)?"
                      r"|sketch_finish_kernel)\(")


@pytest.fixture(scope="module")
def hg():
    import hypergen_amd
    hypergen_amd.lib()
    return hypergen_amd


def library_kernels(hg):
    nm = subprocess.run(["nm", "-C", hg.LIB_PATH], capture_output=True, text=True, check=True).stdout
    return set(FAMILIES.findall(nm))


def test_census_equals_the_library(hg):
    lib = library_kernels(hg)
    names = [r.name for r in sc.ROWS]
    dup = sorted({n for n in names if names.count(n) > 1})
    assert not dup, "rows listed twice: %s" % dup
    for r in sc.ROWS:
        if r.unreachable is not None:
            print("unreachable: %s -- %s" % (r.name, r.unreachable))
    missing = sorted(lib - set(names))
    stale = sorted(set(names) - lib)
    assert not missing, "instantiations in the library without a census row: %s" % missing
    assert not stale, "census rows whose kernel the library does not contain: %s" % stale
    assert len(lib) == len(names) == 14


def test_census_rows_are_routed(hg):
    for r in sc.ROWS:
        assert r.entry in sc.ENTRIES, r
        assert set(r.debug) <= {"sort_test_buckets", "sketch_path"}, r
        assert r.inputs and (r.unreachable is None), r


# ---- the mirror against the plan ------------------------------------------------------------------------------------------
def test_mirror_reads_the_plan(hg):
    """per-genome hit regions from one-genome plans add up to the batch's slots, and their largest is the batch's max_cap"""
    for k, scaled, lens in ((21, 40, [1408, 22 * 513, 22 * 8193, 30_020]), (21, 1500, [30, 21, 20, 1408, 5_000_000]),
                            (33, 1, [100_000, 40, 34])):
        d, _ = hg.sketch_plan_describe(sc.offsets_for(lens), lens, k, scaled)
        max_cap, max_expect, caps = sc.describe(hg, lens, k, scaled)
        assert sum(caps) == d["hit_slots"] and max(caps) == max_cap == d["max_cap"] and max_expect == d["max_expect"]
        for L, c in zip(lens, caps):
            starts = max(0, L - k + 1)
            want = max(1, min(2 * (starts // scaled) + 1024, starts))
            assert c == (want if want <= sc.LDS_MAX_KEYS else sc.pow2_at_least(want)), (L, c)


def test_mirror_sort_launches_follow_the_plan(hg):
    # a batch of few-kbp genomes: the step's count-sized sort holds <= 64 keys (one wave per genome), and a genome of 33..64 raw
    # keys is sorted by the wave kernel and again by the rest launch
    lens = [22 * 40 + 20, 22 * 65, 2_000]
    m = sc.dispatch(hg, "sketch_batch_dev", lens, [40, 65, 1], [40, 65, 1], 21, 1500, 4096, 1)
    assert m.path == "sync_free" and m.sort == ["sort_unique_wave_kernel", "sort_unique_rest_kernel"]
    assert m.sort_branch[0][0] == "sort_unique_wave_kernel+sort_unique_rest_kernel"
    assert m.sort_branch[1][0] == "sort_unique_rest_kernel" and m.sort_branch[2] == ("sort_unique_wave_kernel", "trivial")
    # (every region holds 1 024 keys: the eight-wave encoder is queued for sets the wave kernel leaves, and finds none)
    assert m.encode == ["encode_wave_kernel", "encode_kernel<false>", "sketch_finish_kernel"]
    # a 30 kbp genome expects 20 hits: 20 + 2 + 24 = 46 keys -> 64, no double sort
    m = sc.dispatch(hg, "sketch_batch_dev", [30_020, 22 * 64], [20, 64], [20, 64], 21, 1500, 4096, 1)
    assert m.sort[0] == "sort_unique_wave_kernel" and m.sort_branch[1] == ("sort_unique_wave_kernel", "wave")
    # the largest expected count decides whether the step can go without the host: 7 225 + 903 + 64 = 8 192, 7 226 + 903 + 64 > 8 192
    for expect, path in ((7225, "sync_free"), (7226, "sync")):
        L = expect * 40 + 20
        _, mx, _ = sc.describe(hg, [L], 21, 40)
        assert mx == expect
        assert sc.dispatch(hg, "sketch_batch_dev", [L], [10], [10], 21, 40, 4096, 1).path == path
    # a genome beyond the one-workgroup sort sends the step to the synchronous path: the bucketed chain
    L = 22 * 8193
    m = sc.dispatch(hg, "sketch_batch_dev", [L], [8193], [8193], 21, 40, 4096, 1)
    assert m.path == "sync" and m.sort[1:] == ["bucket_count_kernel", "bucket_scan_kernel", "bucket_scatter_kernel",
                                                 "bucket_sort_kernel", "bucket_scan_kernel", "bucket_copy_kernel"]
    m = sc.dispatch(hg, "sketch_batch_dev", [L], [8192], [8192], 21, 40, 4096, 1)
    assert m.path == "sync_free" and m.sort_branch[0][0] in ("sort_unique_kernel<true>", "sort_unique_rest_kernel")


def test_mirror_encode_launches_follow_the_batch(hg):
    for n, wave_max in ((8191, 256), (8192, 16368)):
        lens = [22] * n
        raw = [1] * n
        m = sc.dispatch(hg, "sketch_batch_dev", lens, raw, raw, 21, 40, 1000, 1)
        assert m.encode == ["encode_wave_kernel", "sketch_finish_kernel"]  # (max_cap 1: no genome can exceed wave_max)
        assert m.encode_branch[0] == ("encode_wave_kernel", "lds4/tail") or m.encode_branch[0][1].endswith("/tail")
        assert sc.encode_branch(wave_max, n, 1000, 1, True, 1 << 20, False)[0] == "encode_wave_kernel"
        assert sc.encode_branch(wave_max + 1, n, 1000, 1, True, 1 << 20, False)[0] == "encode_kernel<false>"
    # raw counts over the slab: the split launch and its finaliser, also for a genome whose distinct count is under the slab
    lens = [22 * 33000, 22 * 40000]
    m = sc.dispatch(hg, "sketch_batch_dev", lens, [33000, 40000], [20000, 40000], 21, 40, 4096, 0)
    assert m.path == "sync" and m.encode == ["encode_wave_kernel", "encode_kernel<false>", "encode_kernel<true>",
                                             "encode_finalize_kernel"]
    assert m.encode_branch == [("encode_kernel<false>", "block+finalize"), ("encode_kernel<true>", "slabs+finalize")]
    # hv_encode: one genome, the wave kernel takes up to 256 hashes
    for n, enc in ((256, ["encode_wave_kernel"]), (257, ["encode_wave_kernel", "encode_kernel<false>"])):
        assert sc.dispatch(hg, "hv_encode", None, None, [n], 0, 0, 64, 1).encode == enc
    # the plane count of the wave kernel and its stores
    assert [sc.encode_branch(d, 1, 4096, 1, True, 0, False)[1] for d in (15, 16, 63, 64, 255, 256)] == \
        ["lds4", "p6/vec", "p6/vec", "p8/vec", "p8/vec", "p14/vec"]
    assert sc.encode_branch(15, 1, 4096, 1, False, 0, False)[1] == "p4/plain"
    assert sc.encode_branch(15, 1, 100, 0, True, 0, False)[1] == "scalar14/plain/tail"


def test_counting_sort_bucket_mirror():
    """17 keys inside one bucket's value range overflow the counting sort; 16 do not"""
    thr = sc.M64 // 40
    n, keys = 600, 1024
    n2 = 1024
    width = thr // n2
    rng = np.random.default_rng(1)
    base = [int(x) for x in rng.choice(np.arange(n2, dtype=np.int64), n - 17, replace=False) * width + width // 2]
    base = [b for b in base if b // width != 7]
    for extra, over in ((16, False), (17, True)):
        hs = base[: n - extra] + [7 * width + 1 + i * (width // 20) for i in range(extra)]
        assert sc.counting_sort_over(hs, n, keys, thr) == over
