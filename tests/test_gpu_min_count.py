"""hg_sketch_params.min_count on the device: kept = the sampled hashes that occur at least m times among a sequence's sampled k-mer
positions.  Everything is compared with `==` against tests/min_count_ref.py (np.unique with counts over the oracle's raw hashes,
then the oracle's encoder), in both input forms of the k-mer kernels (kmer_input = "" / "packed").

Inputs are "dirty" genomes as in test_gpu_set_encode_census.py: distinct sampled k-mers picked with the oracle's hash, each
followed by an N, repeated to plant exact multiplicities -- raw and kept counts are known by construction and confirmed by the
oracle.  Launch lists are those of the host mirror (set_encode_census.dispatch, which mirrors min_count <= 1) with the twins of
tests/min_count_census.py swapped in.
"""
import ctypes
import subprocess

import numpy as np
import pytest
import torch

import min_count_census as mc
import min_count_ref as ref
import set_encode_census as sc

pytestmark = pytest.mark.gpu
K = 21
MAX = 2**64 - 1
ACGT = np.frombuffer(b"ACGT", np.uint8)
N = ord("N")
PENDING = 0xFFFFFFFF
MS = (1, 2, 3, 5, 64, 65, 1000)


@pytest.fixture(scope="module")
def hg():
    import hypergen_amd
    return hypergen_amd


@pytest.fixture(params=["ascii", "packed"])
def form(request):
    return {"kmer_input": "packed"} if request.param == "packed" else {}


_POOLS = {}


def pool(orc, scaled, n):
    """(kmers[n, K], hashes[n]): distinct k-mers whose hash is below the threshold of `scaled`, uniform below it"""
    key = (scaled, n)
    if key not in _POOLS:
        rng = np.random.default_rng(8800 + scaled)
        seq = rng.choice(ACGT, int(n * scaled * 1.25) + 10_000)
        h = orc.kmer_hash_sample(seq, K, threshold=MAX, unique=False)  # pure ACGT: hash i = window i
        idx = np.flatnonzero(h < np.uint64(MAX // scaled))
        _, first = np.unique(h[idx], return_index=True)
        idx = np.sort(idx[first])
        assert idx.size >= n, (scaled, idx.size, n)
        idx = idx[:n]
        _POOLS[key] = (seq[idx[:, None] + np.arange(K)], h[idx])
    return _POOLS[key]


def dirty(kmers, idx):
    """one genome: the k-mers idx (repeats allowed), each followed by an N (the last one's dropped)"""
    sel = kmers[np.asarray(idx, np.int64)]
    return np.concatenate([sel, np.full((len(sel), 1), N, np.uint8)], axis=1).reshape(-1)[:-1].copy()


def planted(kmers, idx, mult, rng):
    """k-mer idx[i] exactly mult[i] times, in random order"""
    return dirty(kmers, rng.permutation(np.repeat(np.asarray(idx, np.int64), np.asarray(mult, np.int64))))


def by_hash(hashes, idx):
    """idx ordered by the k-mers' hash values: position in the sorted list = position here"""
    idx = np.asarray(idx, np.int64)
    return idx[np.argsort(hashes[idx], kind="stable")]


def upload(seqs):
    offs = sc.offsets_for([len(s) for s in seqs])
    host = np.zeros(int(offs[-1]) + len(seqs[-1]) + 80, np.uint8)
    for o, s in zip(offs, seqs):
        host[int(o):int(o) + len(s)] = s
    return torch.from_numpy(host).cuda(), offs, np.array([len(s) for s in seqs], np.uint64)


def outputs(n, hv_d=4096):
    dev = torch.device("cuda:0")
    return (torch.full((n, hv_d), 7, dtype=torch.int16, device=dev), torch.full((n,), 7, dtype=torch.int32, device=dev),
            torch.full((n,), 7, dtype=torch.int32, device=dev))


def want_rows(orc, seqs, m, scaled, hv_d=4096, **kw):
    return [ref.sketch(orc, s, m, K, scaled, hv_d=hv_d, **kw) for s in seqs]


def assert_rows(want, hv, n2, nh):
    hv, n2, nh = np.asarray(hv), np.asarray(n2), np.asarray(nh).view(np.uint32)
    for i, (w_hv, w_n2, w_nh, _) in enumerate(want):
        assert nh[i] == w_nh, (i, int(nh[i]), w_nh)
        assert n2[i] == w_n2, i
        assert np.array_equal(hv[i], w_hv), i


def run_step(hg, orc, seqs, m, scaled, debug=None, ctx=None, hv_d=4096, mirror=True):
    """hg_sketch_batch_dev under min_count = m on a fresh ctx (or `ctx`), resolved with hg_ctx_sync, checked against the reference
    and (mirror) against the launch list of the mirror; returns (the mirror's dispatch, the sort launches reported)"""
    own = ctx is None
    c = hg.Context(0) if own else ctx
    try:
        for kk, v in (debug or {}).items():
            c.set_debug(kk, v)
        d_seq, offs, lens = upload(seqs)
        hv, n2, nh = outputs(len(seqs), hv_d)
        p = hg.default_params(scaled=scaled, hv_d=hv_d, min_count=m)
        c.sketch_batch_dev(d_seq.data_ptr(), offs, lens, p, hv.data_ptr(), n2.data_ptr(), nh.data_ptr())
        c.sync()
        assert_rows(want_rows(orc, seqs, m, scaled, hv_d), hv.cpu().numpy(), n2.cpu().numpy(), nh.cpu().numpy())
        launched = c.last_kernel("sort").split(" + ")
        d = None
        if mirror:
            raws = [orc.kmer_hash_sample(s, K, scaled, unique=False) for s in seqs]
            mdebug = {k: v for k, v in (debug or {}).items() if k != "kmer_input"}
            d = sc.dispatch(hg, "sketch_batch_dev", lens, [r.size for r in raws], [np.unique(r).size for r in raws], K, scaled,
                            hv_d, 1, debug=mdebug, hashes=raws)
            assert launched == mc.sort_launches(d.sort, m), (launched, d.sort)
            assert c.last_kernel("encode") == " + ".join(d.encode)  # (sized by the raw counts: the same for every m)
        return d, launched
    finally:
        if own:
            c.close()


# ---- every row of the census ------------------------------------------------------------------------------------------------
def census_input(orc, name, rng):
    """(seqs, scaled, debug) whose step launches the row under min_count = 2, with multiplicities 1, 2 and 3 in every genome"""
    if name in ("tiny",):
        kmers, _ = pool(orc, 1500, 600)
        seqs = [planted(kmers, np.arange(a, a + d), rng.integers(1, 4, d), rng) for a, d in ((0, 1), (10, 9), (40, 25), (120, 30))]
        seqs.append(rng.choice(ACGT, 30_020))
        return seqs, 1500, {}
    kmers, _ = pool(orc, 40, 34_000)
    if name == "lds":
        return [planted(kmers, np.arange(a, a + d), rng.integers(1, 4, d), rng) for a, d in ((0, 300), (1000, 1500))], 40, {}
    if name == "outgrow":
        shapes = ((0, 2000, 2), (3000, 100, 3), (4000, 1000, 2))
        return [planted(kmers, np.arange(a, a + d), rng.integers(1, hi + 1, d), rng) for a, d, hi in shapes], 40, {}
    if name == "large":
        return [planted(kmers, np.arange(0, 9000), rng.integers(1, 4, 9000), rng),
                planted(kmers, np.arange(10_000, 14_097), np.full(4097, 2), rng)], 40, {"sketch_path": "sync"}
    if name == "inplace":  # two buckets of ~7 000 distinct keys each: more than the 6 144 the counting table takes
        return [planted(kmers, np.arange(0, 14_000), rng.integers(1, 4, 14_000), rng)], 40, {"sort_test_buckets": "2"}
    raise AssertionError(name)


@pytest.mark.parametrize("row", mc.ROWS, ids=[r.name for r in mc.ROWS])
def test_every_census_row_runs(hg, orc, form, row):
    rng = np.random.default_rng(21)
    cls = {"min_count_wave_kernel": "tiny", "min_count_kernel<true>": "lds", "min_count_rest_kernel": "outgrow",
           "min_count_bucket_kernel": "large", "min_count_kernel<false>": "inplace"}[row.name]
    assert cls in row.inputs
    seqs, scaled, debug = census_input(orc, cls, rng)
    assert {k: v for k, v in debug.items() if k != "sketch_path"} == row.debug
    d, launched = run_step(hg, orc, seqs, 2, scaled, dict(debug, **form))
    assert row.name in launched
    assert d.path == ("sync_free" if row.entry == "sketch_batch_dev" else "sync")
    if cls == "inplace":
        assert d.sort_branch[0] == ("sort_unique_kernel<false>", "bucket_lds/gave_up")


# ---- multiplicity edges -------------------------------------------------------------------------------------------------------
def edge_genomes(orc, m, rng):
    """runs of exactly m - 1, m, m + 1; the surviving run first / last in the sorted list; a run across the 512-key chunk of the
    keep-flag scan; all keys equal; nothing survives"""
    kmers, hashes = pool(orc, 40, 12_000)
    seqs = []
    seqs.append(planted(kmers, [0, 1, 2, 3, 4], [max(m - 1, 1), m, m + 1, 1, 1], rng))
    others = 39 if m <= 5 else 3  # (every genome stays within the 8 192 keys of the one-workgroup sort)
    order = by_hash(hashes, np.arange(100, 101 + others))
    low = max(m - 1, 1)
    seqs.append(planted(kmers, order, [m] + [low] * others, rng))            # the survivor is s[0..m)
    seqs.append(planted(kmers, order, [low] * others + [m], rng))            # the survivor ends the list
    seqs.append(planted(kmers, order, [m] + [low] * (others - 1) + [m], rng))
    # singles below the run so that it starts before index 512 and ends behind it
    before = max(0, 512 - max(1, m // 2))
    order = by_hash(hashes, np.arange(1000, 1000 + before + 1 + 30))
    seqs.append(planted(kmers, order, [1] * before + [m] + [1] * 30, rng))
    seqs.append(planted(kmers, order, [1] * before + [m + 1] + [1] * 30, rng))
    if m > 1:
        seqs.append(planted(kmers, order, [1] * before + [m - 1] + [1] * 30, rng))  # ... one short: nothing survives
    seqs.append(planted(kmers, [7], [m], rng))                           # all keys equal: exactly m, and many more
    seqs.append(planted(kmers, [8], [m + 700], rng))
    if m > 1:
        seqs.append(planted(kmers, [9], [m - 1], rng))
    seqs.append(dirty(kmers, np.arange(2000, 2300)))                     # singles only
    return seqs


@pytest.mark.parametrize("m", MS)
def test_multiplicity_edges(hg, orc, form, m):
    rng = np.random.default_rng(100 + m)
    seqs = edge_genomes(orc, m, rng)
    want = want_rows(orc, seqs, m, 40)
    assert [w[2] for w in want[:4]] == ([5, 40, 40, 40] if m == 1 else [2, 1, 1, 2])
    assert all(orc.kmer_hash_sample(s, K, 40, unique=False).size <= 8192 for s in seqs)
    assert want[-1][2] == (300 if m == 1 else 0)
    d, launched = run_step(hg, orc, seqs, m, 40, dict(form))
    assert launched[0] == ("sort_unique_kernel<true>" if m == 1 else "min_count_kernel<true>")


def counted_genome(kmers, raw, m, rng, first=0):
    """exactly `raw` raw hits: runs of m, of m + 1 and of max(m - 1, 1), then singles for the remainder"""
    mult, left = [], raw
    for run in (m, m + 1, max(m - 1, 1)) * 400:
        if run > left:
            break
        mult.append(run)
        left -= run
        if len(mult) >= 3 and m > 8:
            break
    mult += [1] * left
    return planted(kmers, np.arange(first, first + len(mult)), mult, rng) if mult else np.frombuffer(b"ACGTACGTAC", np.uint8).copy()


@pytest.mark.parametrize("m", MS)
def test_raw_count_edges(hg, orc, form, m):
    """raw counts 0, 1, 64, 65, 511, 512, 8 192 in one sync-free step, and 8 193 (beyond the one-workgroup sort: flagged by the
    step, run again through the bucket chain)"""
    kmers, _ = pool(orc, 40, 12_000)
    rng = np.random.default_rng(200 + m)
    seqs = [counted_genome(kmers, raw, m, rng) for raw in (0, 1, 64, 65, 511, 512, 8192)]
    for s, raw in zip(seqs, (0, 1, 64, 65, 511, 512, 8192)):
        assert orc.kmer_hash_sample(s, K, 40, unique=False).size == raw
    with hg.Context(0) as c:
        d, launched = run_step(hg, orc, seqs, m, 40, dict(form), ctx=c)
        assert d.path == "sync_free" and c.sketch_step_counts()[2] == 0
    seqs = [counted_genome(kmers, 8193, m, rng), counted_genome(kmers, 300, m, rng)]
    with hg.Context(0) as c:
        d, launched = run_step(hg, orc, seqs, m, 40, dict(form), ctx=c)
        assert c.sketch_step_counts() == (1, 1, 1) and d.path == "sync"
        assert ("bucket_sort_kernel" if m == 1 else "min_count_bucket_kernel") in launched


@pytest.mark.parametrize("crowd", (16, 17))
def test_counting_sort_give_up_edge(hg, orc, form, crowd):
    """600 raw keys under m = 2 with 16 / 17 of them in one counting-sort bucket (eight doubled k-mers, and one more): with 17 the
    counting sort gives up and the bitonic network sorts"""
    kmers, hashes = pool(orc, 40, 12_000)
    rng = np.random.default_rng(300 + crowd)
    lens = [22 * 600 - 1]
    m0 = sc.dispatch(hg, "sketch_batch_dev", lens, [1], [1], K, 40, 4096, 1)
    keys = m0.keys[0] if 600 <= m0.keys[0] else m0.keys[1]
    b = np.array([sc.sort_bucket(int(h), 1024, keys, MAX // 40) for h in hashes])
    target = int(np.bincount(b).argmax())
    inside = np.flatnonzero(b == target)
    assert inside.size >= 9
    idx, mult, per = list(inside[:8]), [2] * 8, {}
    if crowd == 17:
        idx.append(inside[8]), mult.append(1)
    for i in rng.permutation(np.flatnonzero(b != target)):
        left = 600 - sum(mult)
        if left == 0:
            break
        if per.get(b[i], 0) < 4:
            per[b[i]] = per.get(b[i], 0) + 1
            idx.append(i), mult.append(2 if left >= 2 else 1)
    assert sum(mult) == 600
    seq = planted(kmers, idx, mult, rng)
    assert len(seq) == lens[0]
    d, launched = run_step(hg, orc, [seq], 2, 40, dict(form))
    assert d.sort_branch[0][1] == ("counting" if crowd == 16 else "counting>bitonic")
    assert launched[0] == "min_count_kernel<true>"


# ---- the bucket chain ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", (2, 3))
def test_bucket_chain_table_and_in_place(hg, orc, form, m):
    kmers, _ = pool(orc, 40, 34_000)
    rng = np.random.default_rng(400 + m)
    base = np.arange(0, 9000)
    seqs = [planted(kmers, np.arange(10_000, 30_000), rng.integers(1, 3, 20_000), rng),      # ~30 000 raw, 20 000 distinct
            planted(kmers, base, rng.integers(1, 5, 9000), rng)]                             # ~22 500 raw, 9 000 distinct
    d, launched = run_step(hg, orc, seqs, m, 40, dict(form, sketch_path="sync"))
    assert [b[1] for b in d.sort_branch] == ["bucket_lds", "bucket_lds"] and "min_count_bucket_kernel" in launched
    # 4 096 buckets: counted and scattered through global memory
    d, launched = run_step(hg, orc, seqs[1:], m, 40, dict(form, sort_test_buckets="4096"))
    assert d.sort_branch[0] == ("bucket_sort_kernel", "bucket_global")
    # 2 buckets of > 8 192 keys: the counting table takes the 4 500 distinct keys of a bucket; with 10 000 it overflows and
    # the in-place kernel finishes the genome
    d, launched = run_step(hg, orc, seqs, m, 40, dict(form, sort_test_buckets="2"))
    assert d.sort_branch[0] == ("sort_unique_kernel<false>", "bucket_lds/gave_up")
    assert d.sort_branch[1] == ("bucket_sort_kernel", "bucket_lds/hashset")
    assert launched[-1] == "min_count_kernel<false>" and "min_count_bucket_kernel" in launched


def test_bucket_of_mostly_distinct_keys_falls_back_to_the_sorted_filter(hg, orc, form):
    """two buckets of ~7 000 raw keys each, ~6 500 of them distinct: they fit the 8 192 keys of LDS, but not the 6 144 distinct
    keys the counting table takes -- the bucket is sorted whole and filtered by the look-ahead"""
    kmers, hashes = pool(orc, 40, 34_000)
    rng = np.random.default_rng(440)
    seq = planted(kmers, np.arange(0, 13_000), [2] * 700 + [3] * 300 + [1] * 12_000, rng)
    thr = MAX // 40
    mul = min(((2 << 64) + thr - 1) // thr, MAX)
    for b in (0, 1):
        inside = np.array([min((int(h) * mul) >> 64, 1) == b for h in hashes[:13_000]])
        raw = int(np.where(inside, np.array([2] * 700 + [3] * 300 + [1] * 12_000), 0).sum())
        assert 4096 < raw <= 8192 and inside.sum() > 6144, (b, raw, inside.sum())
    for m in (2, 3):
        d, launched = run_step(hg, orc, [seq], m, 40, dict(form, sort_test_buckets="2"))
        assert d.sort_branch[0] == ("bucket_sort_kernel", "bucket_lds") and launched[-1] == "bucket_copy_kernel"
        assert ref.sketch(orc, seq, m, K, 40)[2] == (1000 if m == 2 else 300)


def test_split_encode_of_a_set_far_smaller_than_its_raw_count(hg, orc, form):
    """the slab split of the encoders is planned from raw counts: genomes of > 32 768 raw hits of which few, or none, survive"""
    kmers, _ = pool(orc, 40, 34_000)
    rng = np.random.default_rng(450)
    seqs = [dirty(kmers, np.arange(0, 33_000)),                                                       # m = 2: nothing survives
            planted(kmers, np.arange(0, 33_000), [2] * 100 + [1] * 32_900, rng),                      # 100 survive
            planted(kmers, np.arange(0, 17_000), [2] * 17_000, rng)]                                  # 17 000 survive
    d, launched = run_step(hg, orc, seqs, 2, 40, dict(form))
    assert d.encode[-2:] == ["encode_kernel<true>", "encode_finalize_kernel"]


# ---- a hit region that overflows -------------------------------------------------------------------------------------------
R = 5000


def overflowing(orc, rng):
    """one sampled k-mer + N planted R times (110 kbp: its region holds 2 * 73 + 1 024 hits at scaled = 1 500), beside k-mers
    planted once and twice"""
    kmers, _ = pool(orc, 1500, 600)
    unit = np.concatenate([kmers[0], [N]]).astype(np.uint8)
    extra = planted(kmers, [1, 2, 3, 4, 5], [1, 2, 1, 2, 2], rng)
    seq = np.concatenate([np.tile(unit, R), extra])
    raw = orc.kmer_hash_sample(seq, K, 1500, unique=False)
    assert raw.size == R + 8 and raw.size > 2 * (len(seq) // 1500) + 1024
    return seq


@pytest.mark.parametrize("path", ("sync_free", "sync"))
def test_overflowing_region_is_counted_whole(hg, orc, form, path):
    rng = np.random.default_rng(500)
    seqs = [overflowing(orc, rng), rng.choice(ACGT, 90_000)]
    for m, nhash in ((R, 1), (R + 1, 0), (2, 4), (1, 6)):
        assert ref.sketch(orc, seqs[0], m, K, 1500)[2] == nhash
        with hg.Context(0) as c:
            debug = dict(form, sketch_path="sync") if path == "sync" else dict(form)
            run_step(hg, orc, seqs, m, 1500, debug, ctx=c, mirror=False)
            # sync-free: the check word sent the step through the synchronous path, which grew the region and ran again
            assert c.sketch_step_counts() == ((1, 1, 1) if path == "sync_free" else (0, 1, 0))


def test_stream_ordered_consumer_sees_final_rows_or_pending(hg, orc, form):
    rng = np.random.default_rng(510)
    seqs = [rng.choice(ACGT, 150_000), overflowing(orc, rng), planted(pool(orc, 1500, 600)[0], np.arange(100, 130),
                                                                      rng.integers(1, 4, 30), rng)]
    want = want_rows(orc, seqs, 2, 1500)
    with hg.Context(0) as c:
        for kk, v in form.items():
            c.set_debug(kk, v)
        d_seq, offs, lens = upload(seqs)
        hv, n2, nh = outputs(3)
        c.sketch_batch_dev(d_seq.data_ptr(), offs, lens, hg.default_params(min_count=2), hv.data_ptr(), n2.data_ptr(), nh.data_ptr())
        torch.cuda.synchronize()  # the stream alone: NOT the library's completion point
        got = nh.cpu().numpy().view(np.uint32)
        assert got[1] == PENDING and bool((hv[1] == 7).all())
        for i in (0, 2):
            assert got[i] == want[i][2] and np.array_equal(hv[i].cpu().numpy(), want[i][0])
        c.sync()
        assert c.sketch_step_counts() == (1, 1, 1)
        assert_rows(want, hv.cpu().numpy(), n2.cpu().numpy(), nh.cpu().numpy())


# ---- every entry point -----------------------------------------------------------------------------------------------------
def mixed_batch(orc, rng):
    kmers, _ = pool(orc, 40, 12_000)
    return [planted(kmers, np.arange(0, 40), rng.integers(1, 4, 40), rng),
            planted(kmers, np.arange(100, 1300), rng.integers(1, 5, 1200), rng),
            planted(kmers, np.arange(2000, 7000), rng.integers(1, 4, 5000), rng),      # ~10 000 raw: the bucket chain
            rng.choice(ACGT, 60_000), np.frombuffer(b"ACGTNACG", np.uint8).copy(),
            planted(kmers, [7000], [300], rng)]


@pytest.mark.parametrize("m", (2, 3))
def test_every_entry_point_gives_the_same_rows(hg, orc, m):
    rng = np.random.default_rng(600 + m)
    seqs = mixed_batch(orc, rng)
    n = len(seqs)
    p = hg.default_params(scaled=40, min_count=m)
    want = want_rows(orc, seqs, m, 40)
    assert sum(w[2] for w in want) > 2000 and want[4][2] == 0  # (the reference's own counts: the batch is not trivial)
    rows = {}
    with hg.Context(0) as c:
        d_seq, offs, lens = upload(seqs)
        hv, n2, nh = outputs(n)
        c.sketch_batch_dev(d_seq.data_ptr(), offs, lens, p, hv.data_ptr(), n2.data_ptr(), nh.data_ptr())
        c.sync()
        rows["dev"] = (hv.cpu().numpy(), n2.cpu().numpy(), nh.cpu().numpy())
        blobs = [hg.pack2(s) for s in seqs]
        d_blobs, boffs, _ = upload(blobs)
        hv, n2, nh = outputs(n)
        c.sketch_batch_dev_packed(d_blobs.data_ptr(), boffs, lens, p, hv.data_ptr(), n2.data_ptr(), nh.data_ptr())
        c.sync()
        assert c.last_kernel("kmer").endswith("true>")
        rows["dev_packed"] = (hv.cpu().numpy(), n2.cpu().numpy(), nh.cpu().numpy())
        for hostfed in ("ascii", "packed"):
            c.set_debug("hostfed", hostfed)
            rows["batch_" + hostfed] = c.sketch_batch(seqs, p)
        c.set_debug("hostfed", "")
        for i, s in enumerate(seqs):
            got = c.kmer_hash_sample(s, K, 40, min_count=m)
            assert got.dtype == np.uint64 and np.array_equal(got, want[i][3]), i
        # the capacity rule: one slot short -> HG_ERR_CAPACITY and the kept count
        s = np.ascontiguousarray(seqs[1])
        out = np.zeros(want[1][2], np.uint64)
        n_out = ctypes.c_size_t(0)
        args = (c._h, ctypes.c_void_p(s.ctypes.data), s.size, K, ctypes.c_uint64(MAX // 40), ctypes.c_uint64(123), 1, 0, m,
                ctypes.c_void_p(out.ctypes.data))
        assert hg.lib().hg_kmer_hash_sample_min_count(*args, want[1][2] - 1, ctypes.byref(n_out)) == hg.ERR_CAPACITY
        assert n_out.value == want[1][2]
        assert hg.lib().hg_kmer_hash_sample_min_count(*args, want[1][2], ctypes.byref(n_out)) == hg.OK
        assert n_out.value == want[1][2] and np.array_equal(out, want[1][3])
    for kind in ("ascii", "packed", "sparse"):
        with hg.SketchStream([0], p) as st:
            for i, s in enumerate(seqs):
                if kind == "ascii":
                    st.push(s, i)
                elif kind == "packed":
                    st.push_packed(hg.pack2(s), len(s), i)
                else:
                    blob = hg.pack2s(s)
                    assert blob is not None or i in (0, 1, 2, 5)  # (a dirty genome has an N every 22 bases: no sparse form)
                    st.push_packed_sparse(blob, len(s), i) if blob is not None else st.push(s, i)
            st.finish()
            seen = {}
            while True:
                r = st.pop()
                if r is None:
                    break
                seen[r[0]] = r[1:]
        assert sorted(seen) == list(range(n))
        rows["stream_" + kind] = (np.stack([seen[i][0] for i in range(n)]), np.array([seen[i][1] for i in range(n)]),
                                  np.array([seen[i][2] for i in range(n)], np.uint32))
    with hg.Multi([0, 0]) as mu:
        rows["multi"] = mu.sketch_batch(seqs, p)
    for name, (hv, n2, nh) in rows.items():
        assert_rows(want, hv, n2, nh)


def test_min_count_0_and_1_are_the_default(hg, orc, form):
    rng = np.random.default_rng(700)
    cases = [(mixed_batch(orc, rng), 40, {}), (census_input(orc, "tiny", rng)[0], 1500, {}),
             (census_input(orc, "inplace", rng)[0], 40, {"sort_test_buckets": "2"})]
    for seqs, scaled, debug in cases:
        got = []
        for p in (hg.default_params(scaled=scaled), hg.default_params(scaled=scaled, min_count=0), hg.default_params(scaled=scaled, min_count=1)):
            with hg.Context(0) as c:
                for kk, v in dict(debug, **form).items():
                    c.set_debug(kk, v)
                d_seq, offs, lens = upload(seqs)
                hv, n2, nh = outputs(len(seqs))
                c.sketch_batch_dev(d_seq.data_ptr(), offs, lens, p, hv.data_ptr(), n2.data_ptr(), nh.data_ptr())
                c.sync()
                got.append((hv.cpu().numpy(), n2.cpu().numpy(), nh.cpu().numpy(), c.last_kernel("sort"), c.last_kernel("encode"),
                            c.sketch_step_counts()))
        assert "min_count" not in got[0][3]
        for g in got[1:]:
            assert np.array_equal(g[0], got[0][0]) and np.array_equal(g[1], got[0][1]) and np.array_equal(g[2], got[0][2])
            assert g[3:] == got[0][3:]
        for i, s in enumerate(seqs):
            w_hv, w_n2, w_nh = orc.sketch_genome(s, K, scaled)
            assert got[0][2].view(np.uint32)[i] == w_nh and got[0][1][i] == w_n2 and np.array_equal(got[0][0][i], w_hv)


# ---- the read set ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def reads():
    return ref.read_set()


def test_read_set_against_its_genome(hg, orc, form, reads):
    """30x reads of a 300 kbp genome, 1 % substitutions, both strands (37 535 raw hits at scaled = 200: the bucket chain): the
    kept sets, HVs and norms for m = 1..4, and the ANI of each against the genome's own sketch"""
    buf, genome = reads
    with hg.Context(0) as c:
        for kk, v in form.items():
            c.set_debug(kk, v)
        ghv, gn2, gnh = c.sketch_batch([genome], hg.default_params(scaled=200))
        assert gnh[0] == 1431
        anis = []
        for m in (1, 2, 3, 4):
            w_hv, w_n2, w_nh, w_kept = ref.sketch(orc, buf, m, K, 200)
            assert np.array_equal(c.kmer_hash_sample(buf, K, 200, min_count=m), w_kept)
            d_seq, offs, lens = upload([buf])
            hv, n2, nh = outputs(1)
            c.sketch_batch_dev(d_seq.data_ptr(), offs, lens, hg.default_params(scaled=200, min_count=m), hv.data_ptr(), n2.data_ptr(),
                               nh.data_ptr())
            c.sync()
            assert ("bucket_sort_kernel" if m == 1 else "min_count_bucket_kernel") in c.last_kernel("sort").split(" + ")
            hv, n2, nh = hv.cpu().numpy(), n2.cpu().numpy(), nh.cpu().numpy()
            assert_rows([(w_hv, w_n2, w_nh, w_kept)], hv, n2, nh)
            ani = c.dist_full(ghv, gn2, hv, n2, K)
            dot = int(ghv[0].astype(np.int64) @ hv[0].astype(np.int64))
            assert float(ani[0, 0]) == orc.ani_from_dot(dot, int(gn2[0]), int(n2[0]), K)
            anis.append(float(ani[0, 0]))
        assert anis[0] < 96 < 99 < anis[1] < anis[2] <= anis[3] == 100.0


def test_cli_sketch_min_count_then_dist(tmp_path, orc, hg, reads):
    buf, genome = reads
    rd, gd = tmp_path / "reads", tmp_path / "genome"
    rd.mkdir(), gd.mkdir()
    rl = 150
    recs = buf.reshape(-1, rl + 1)[:, 1:]
    with open(rd / "reads.fna", "w") as f:  # FASTQ records (the reader goes by content; the directory scan by suffix)
        for i, r in enumerate(recs):
            f.write("@r%d\n%s\n+\n%s\n" % (i, bytes(r).decode(), "I" * rl))
    with open(gd / "genome.fna", "w") as f:
        f.write(">g\n%s\n" % bytes(genome[1:]).decode())
    rs, gs, tsv = str(tmp_path / "reads.sketch"), str(tmp_path / "genome.sketch"), str(tmp_path / "ani.tsv")
    r = subprocess.run([hg.CLI_PATH, "sketch", "-p", str(rd), "-o", rs, "-s", "200", "--min_count", "2"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([hg.CLI_PATH, "sketch", "-p", str(gd), "-o", gs, "-s", "200"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([hg.CLI_PATH, "dist", "-r", gs, "-q", rs, "-o", tsv, "-a", "0"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    # the model: what the reader hands over (needletail's records, merged), the reference's set of it, the oracle's ANI
    merged = hg.read_merge_seq(str(rd / "reads.fna"), hg.READ_NEEDLETAIL)
    w_hv, w_n2, w_nh, _ = ref.sketch(orc, merged, 2, K, 200, norm=orc.NORM_U2T)
    assert w_nh == 1671
    g_hv, g_n2, _ = orc.sketch_genome(hg.read_merge_seq(str(gd / "genome.fna"), hg.READ_NEEDLETAIL), K, 200, norm=orc.NORM_U2T)
    x = hg.read_sketch_file(rs)[0]
    assert x["hv_norm_2"] == w_n2 and (hg.hv_unpack(x["hv"].view(np.uint8), 4096, x["hv_quant_bits"]) == w_hv).all()
    want = orc.ani_matrix(g_hv[None], np.array([g_n2], np.int32), w_hv[None], np.array([w_n2], np.int32), K)
    assert open(tsv).read() == "%s\t%s\t%.3f\n" % (str(gd / "genome.fna"), str(rd / "reads.fna"), float(want[0, 0]))
    assert 99 < float(want[0, 0]) < 100
