"""Every set-stage and encode-stage kernel (tests/set_encode_census.py), run by genomes planted on its row and at the edges where
its dispatch changes.  Each call is checked three ways: ctx.last_kernel("sort") / ("encode") equals the launch list the host mirror
(set_encode_census.dispatch) predicts, exactly; the mirror sends the planted genome to the row; nhash, the HV row and the norm
equal the oracle's (orc.sketch_genome / orc.encode_hv + orc.hv_norm2) bit for bit, and hash sets equal orc.kmer_hash_sample.

Genomes are "dirty" (tests/sampling_craft.py): distinct sampled k-mers chosen by the oracle's hash, each followed by an N, so a
genome's raw and distinct sampled counts are exactly the planted ones; repeating k-mers sets multiplicities.  Choosing k-mers by
hash value plants 16 or 17 distinct keys in one counting-sort bucket.  hg_hv_encode takes any distinct hashes: there hashes
picked with the oracle's WyRng stream saturate one dimension (its bit is 1 in every hash) and leave another at 0.
"""
import numpy as np
import pytest
import torch

import set_encode_census as sc

pytestmark = pytest.mark.gpu
K = 21
MAX = 2**64 - 1
ACGT = np.frombuffer(b"ACGT", np.uint8)
N = ord("N")
HV_DS = (64, 100, 1000, 4096, 4160, 16384, 32768)


@pytest.fixture(scope="module")
def hg():
    import hypergen_amd
    return hypergen_amd


@pytest.fixture(scope="module")
def mctx(hg):
    c = hg.Context(0)
    yield c
    c.close()


_POOLS = {}


def pool(orc, scaled, n):
    """(kmers[n, K], hashes[n]): distinct k-mers whose hash is below the threshold of `scaled`, uniform below it"""
    key = (scaled, n)
    if key not in _POOLS:
        rng = np.random.default_rng(7700 + scaled)
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


def sampled(orc, seq, scaled):
    raw = orc.kmer_hash_sample(seq, K, scaled, unique=False)
    return raw, np.unique(raw)


def upload(seqs):
    offs = sc.offsets_for([len(s) for s in seqs])
    host = np.zeros(int(offs[-1]) + len(seqs[-1]) + 80, np.uint8)
    for o, s in zip(offs, seqs):
        host[int(o):int(o) + len(s)] = s
    return torch.from_numpy(host).cuda(), offs, np.array([len(s) for s in seqs], np.uint64)


def run_step(hg, orc, seqs, scaled, hv_d=4096, layout=1, debug=None, offset2=False, ctx=None, seen=0, check_oracle=True):
    """hg_sketch_batch_dev on a fresh ctx (or `ctx`), resolved with hg_ctx_sync; returns the mirror's dispatch"""
    own = ctx is None
    c = hg.Context(0) if own else ctx
    try:
        for kk, v in (debug or {}).items():
            c.set_debug(kk, v)
        d_seq, offs, lens = upload(seqs)
        n = len(seqs)
        dev = torch.device("cuda:0")
        buf = torch.full((n * hv_d + 16,), 7, dtype=torch.int16, device=dev)
        hv = buf[1:1 + n * hv_d] if offset2 else buf[8:8 + n * hv_d]  # (8 int16 = 16 bytes: the allocation's alignment kept)
        assert (hv.data_ptr() % 16 == 2) == offset2
        n2 = torch.full((n,), 7, dtype=torch.int32, device=dev)
        nh = torch.full((n,), 7, dtype=torch.int32, device=dev)
        p = hg.default_params(scaled=scaled, hv_d=hv_d, hv_layout=layout)
        c.sketch_batch_dev(d_seq.data_ptr(), offs, lens, p, hv.data_ptr(), n2.data_ptr(), nh.data_ptr())
        c.sync()
        sets = [sampled(orc, s, scaled) for s in seqs]
        m = sc.dispatch(hg, "sketch_batch_dev", lens, [r.size for r, _ in sets], [u.size for _, u in sets], K, scaled, hv_d,
                        layout, aligned=not offset2, debug=debug, seen=seen, hashes=[r for r, _ in sets])
        assert c.last_kernel("sort") == " + ".join(m.sort)
        assert c.last_kernel("encode") == " + ".join(m.encode)
        if check_oracle:
            hv_h = hv.view(n, hv_d).cpu().numpy()
            n2_h, nh_h = n2.cpu().numpy(), nh.cpu().numpy().view(np.uint32)
            for i, s in enumerate(seqs):
                w_hv, w_n2, w_nh = orc.sketch_genome(s, K, scaled, hv_d=hv_d, layout=layout)
                assert nh_h[i] == w_nh == sets[i][1].size, (i, nh_h[i], w_nh)
                assert n2_h[i] == w_n2, i
                assert np.array_equal(hv_h[i], w_hv), i
        return m
    finally:
        if own:
            c.close()


# ---- encode: hg_hv_encode ---------------------------------------------------------------------------------------------------
PLANE_EDGES = (0, 1, 2, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1000)


@pytest.mark.parametrize("layout", (0, 1))
def test_hv_encode_every_plane_count_and_width(hg, mctx, orc, layout):
    rng = np.random.default_rng(31 + layout)
    hashes = np.unique(rng.integers(0, 2**63, 1100, dtype=np.uint64) * np.uint64(2) + np.uint64(1))[:1000]
    rng.shuffle(hashes)
    seen_rows = set()
    for hv_d in HV_DS:
        for n in PLANE_EDGES:
            h = hashes[:n]
            hv, n2 = mctx.hv_encode(h, hv_d, layout)
            m = sc.dispatch(hg, "hv_encode", None, None, [n], 0, 0, hv_d, layout)
            assert mctx.last_kernel("encode") == " + ".join(m.encode), (hv_d, n)
            want = orc.encode_hv(h, hv_d, layout)
            assert np.array_equal(hv, want), (hv_d, n)
            assert n2 == orc.hv_norm2(want), (hv_d, n)
            seen_rows.add(m.encode_branch[0][0])
            if layout == 1 and hv_d == 4096:
                assert m.encode_branch[0][1] == ("lds4" if n < 16 else "p6/vec" if n < 64 else "p8/vec" if n < 256 else
                                                 "p14/vec" if n <= 256 else "block")
    assert seen_rows == {"encode_wave_kernel", "encode_kernel<false>"}


_SATURATING = {}


def saturating_hashes(orc, n):
    """n distinct hashes whose WyRng word 0 has bit 0 set and bit 1 clear: dimension 0 counts every hash, the dimension of
    bit 1 none (position 1 in the scalar order, 4 in the AVX2 order)"""
    if n in _SATURATING:
        return _SATURATING[n]
    rng = np.random.default_rng(99)
    out = []
    while len(out) < n:
        for h in rng.integers(0, 2**63, 4096, dtype=np.uint64):
            w = orc.wyrng_stream(int(h), 1)[0]
            if (w & 3) == 1:
                out.append(int(h))
    out = np.unique(np.array(out[: n + 64], np.uint64))[:n]
    assert out.size == n
    _SATURATING[n] = out
    return out


@pytest.mark.parametrize("layout", (0, 1))
def test_hv_encode_saturated_columns_cross_the_flush_window(hg, mctx, orc, layout):
    """one column at n: counts reach the top of the 14 bit-sliced planes, and at 16 369 + they cross the flush window of
    1 023 blocks of 16 hashes (32 768 dims: one hash slice per wave, every hash in one window run)"""
    allh = saturating_hashes(orc, 32769)
    pos1 = 1 if layout == 0 else 4
    # (below 257 the wave kernel: a column at n needs every plane its plane-count choice keeps)
    for n in (1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 16368, 16369, 32767, 32768, 32769):
        h = allh[:n]
        for hv_d in (32768, 4096):
            hv, n2 = mctx.hv_encode(h, hv_d, layout)
            m = sc.dispatch(hg, "hv_encode", None, None, [n], 0, 0, hv_d, layout)
            assert mctx.last_kernel("encode") == " + ".join(m.encode)
            assert m.encode == (["encode_wave_kernel"] if n <= 256 else ["encode_wave_kernel", "encode_kernel<false>"])
            want = orc.encode_hv(h, hv_d, layout)
            assert int(want[0]) == np.int16(np.uint16(n & 0xFFFF)) and int(want[pos1]) == np.int16(np.uint16(-n & 0xFFFF))
            assert np.array_equal(hv, want), (n, hv_d)
            assert n2 == orc.hv_norm2(want), (n, hv_d)


def test_hv_encode_wraps_the_norm(hg, mctx, orc):
    rng = np.random.default_rng(5)
    h = np.unique(rng.integers(0, 2**64 - 1, 600_000, dtype=np.uint64))
    hv, n2 = mctx.hv_encode(h, 4096, 1)
    want = orc.encode_hv(h, 4096, 1)
    assert int((want.astype(np.int64) ** 2).sum()) > 2**31  # (the i32 sum wraps)
    assert np.array_equal(hv, want) and n2 == orc.hv_norm2(want)
    assert mctx.last_kernel("encode") == "encode_wave_kernel + encode_kernel<false>"


# ---- set stage: the sync-free step -------------------------------------------------------------------------------------------
def bucket_genome(orc, kmers, hashes, n, keys, scaled, crowd, rng):
    """n distinct pool k-mers with `crowd` of them in one counting-sort bucket and at most 8 in every other one"""
    thr = MAX // scaled
    n2 = sc.pow2_at_least(n)
    b = np.array([sc.sort_bucket(int(h), n2, keys, thr) for h in hashes])
    target = int(np.bincount(b).argmax())
    inside = np.flatnonzero(b == target)
    assert inside.size >= crowd
    pick = list(inside[:crowd])
    per = {}
    for i in rng.permutation(np.flatnonzero(b != target)):
        if len(pick) == n:
            break
        if per.get(b[i], 0) < 8:
            per[b[i]] = per.get(b[i], 0) + 1
            pick.append(i)
    assert len(pick) == n
    return dirty(kmers, rng.permutation(pick))


def edge_batch(orc, scaled=40):
    """raw = distinct = 1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, plus 1 500 raw of 1 000 distinct (repeats), and two
    600-key genomes whose counting sort sees 16 / 17 keys in one bucket"""
    kmers, hashes = pool(orc, scaled, 12_000)
    rng = np.random.default_rng(4)
    seqs, off = [], 0
    for n in (1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513):
        seqs.append(dirty(kmers, np.arange(off, off + n)))
        off += n
    rep = np.arange(off, off + 1000)
    seqs.append(dirty(kmers, rng.permutation(np.concatenate([rep, rep[:500]]))))
    return seqs, kmers[off + 1000:], hashes[off + 1000:], rng


@pytest.mark.parametrize("hv_d,layout,offset2", [(4096, 1, False), (4096, 0, False), (64, 1, False), (100, 1, False),
                                                 (1000, 0, False), (4160, 1, False), (16384, 1, False), (32768, 0, False),
                                                 (4096, 1, True), (4160, 0, True)])
def test_sort_edges_in_the_sync_free_step(hg, orc, hv_d, layout, offset2):
    seqs, bk, bh, rng = edge_batch(orc)
    lens = [len(s) for s in seqs] + [22 * 600 - 1] * 2
    # the launch that sorts the 600-key genomes: the mirror says which, and with how many LDS keys
    m0 = sc.dispatch(hg, "sketch_batch_dev", lens, [1] * len(lens), [1] * len(lens), K, 40, hv_d, layout)
    assert m0.path == "sync_free"
    keys = m0.keys[0] if 600 <= m0.keys[0] else m0.keys[1]
    seqs += [bucket_genome(orc, bk, bh, 600, keys, 40, crowd, rng) for crowd in (16, 17)]
    m = run_step(hg, orc, seqs, 40, hv_d, layout, offset2=offset2)
    assert m.path == "sync_free" and m.sort[0] == "sort_unique_kernel<true>"
    br = [b[1].split("/")[-1] for b in m.sort_branch]
    assert br[:3] == ["trivial", "wave", "wave"] and br[4] == "bitonic" and br[8] == "bitonic" and br[9] == "counting"
    assert br[-2:] == ["counting", "counting>bitonic"]
    enc = [b[1] for b in m.encode_branch]
    if layout == 1 and not offset2 and hv_d % 64 == 0:
        assert enc[:8] == ["lds4", "lds4", "p6/vec", "p8/vec", "p8/vec", "p8/vec", "p14/vec", "block"]
    if offset2 or hv_d % 8:
        assert all(e == "block" or "/plain" in e for e in enc)


def test_double_sort_of_sets_between_the_wave_launch_and_64(hg, orc):
    """the count-sized sort holds 32 keys: the wave kernel sorts every set of <= 64 keys, and the rest launch sorts the sets of
    33..64 raw keys again -- their region's tail is what the wave kernel left of the raw keys"""
    kmers, _ = pool(orc, 1500, 600)
    rng = np.random.default_rng(8)
    shapes = [(1, 1), (2, 2), (16, 16), (32, 32), (33, 33), (40, 40), (64, 64), (65, 65), (100, 100), (60, 30), (64, 33),
              (50, 40), (33, 17)]
    seqs, off = [], 0
    for raw, dist in shapes:
        base = np.arange(off, off + dist)
        off += dist
        seqs.append(dirty(kmers, rng.permutation(np.concatenate([base, rng.choice(base, raw - dist)]))))
    m = run_step(hg, orc, seqs, 1500, 4096, 1)
    assert m.path == "sync_free" and m.keys[0] == 32
    assert m.sort == ["sort_unique_wave_kernel", "sort_unique_rest_kernel"]
    doubled = [i for i, b in enumerate(m.sort_branch) if b[0] == "sort_unique_wave_kernel+sort_unique_rest_kernel"]
    assert [shapes[i][0] for i in doubled] == [33, 40, 64, 60, 64, 50, 33]
    # and the same genomes once more as hash sets (the synchronous path, one genome per call)
    for s in seqs[3:8]:
        with hg.Context(0) as c:
            got = c.kmer_hash_sample(s, K, 1500)
            assert np.array_equal(got, orc.kmer_hash_sample(s, K, 1500))


def test_tiny_batch_one_wave_per_genome(hg, orc):
    kmers, _ = pool(orc, 1500, 600)
    rng = np.random.default_rng(9)
    seqs = [dirty(kmers, np.arange(i, i + n)) for i, n in ((0, 1), (10, 20), (40, 64), (120, 63))]
    seqs.append(rng.choice(ACGT, 30_020))  # expects 20 hits: 20 + 2 + 24 -> 64 keys
    m = run_step(hg, orc, seqs, 1500, 1000, 1)
    # (the rest launch is queued for the 1 024-key regions, and finds no genome to take)
    assert m.sort == ["sort_unique_wave_kernel", "sort_unique_rest_kernel"] and m.keys[0] == 64
    assert m.encode[-1] == "sketch_finish_kernel"
    assert all(b[0] == "sort_unique_wave_kernel" for b in m.sort_branch)


def test_genomes_outgrowing_the_count_sized_sort(hg, orc):
    kmers, _ = pool(orc, 40, 12_000)
    seqs = [dirty(kmers, np.arange(0, 3000)), dirty(kmers, np.arange(3000, 3100)), dirty(kmers, np.arange(4000, 6000))]
    m = run_step(hg, orc, seqs, 40, 4096, 1)
    assert m.path == "sync_free" and m.sort == ["sort_unique_kernel<true>", "sort_unique_rest_kernel"]
    assert m.sort_branch[0][0] == "sort_unique_rest_kernel" and m.sort_branch[1][0] == "sort_unique_kernel<true>"


@pytest.mark.parametrize("n_big", (8192, 8193))
def test_one_workgroup_sort_edge_and_the_redo(hg, orc, n_big):
    kmers, _ = pool(orc, 40, 12_000)
    seqs = [dirty(kmers, np.arange(0, n_big)), dirty(kmers, np.arange(9000, 9300))]
    with hg.Context(0) as c:
        f0, s0, r0 = c.sketch_step_counts()
        m = run_step(hg, orc, seqs, 40, 4096, 1, ctx=c)
        f1, s1, r1 = c.sketch_step_counts()
    assert f1 - f0 == 1 and r1 - r0 == (1 if n_big > 8192 else 0)
    if n_big > 8192:  # flagged by the step, run again synchronously: its launches are the ones reported
        assert m.path == "sync" and m.sort_branch[0] == ("bucket_sort_kernel", "bucket_lds")
        assert "bucket_copy_kernel" in m.sort
    else:
        assert m.path == "sync_free" and m.sort_branch[0][1] == "counting"


# ---- set stage: the synchronous path ---------------------------------------------------------------------------------------
def test_sync_path_redo_after_a_count_grew(hg, orc):
    """same geometry twice under sketch_path = sync: the second sort is sized by the first run's counts, and the genome that
    grew past it is sorted again from the host's todo list"""
    kmers, _ = pool(orc, 40, 12_000)
    rng = np.random.default_rng(12)
    grown = dirty(kmers, np.arange(0, 3000))
    small = rng.choice(ACGT, grown.size)
    other = dirty(kmers, np.arange(5000, 5100))
    with hg.Context(0) as c:
        m1 = run_step(hg, orc, [small, other], 40, 4096, 1, debug={"sketch_path": "sync"}, ctx=c)
        seen = max(sampled(orc, s, 40)[0].size for s in (small, other))
        m2 = run_step(hg, orc, [grown, other], 40, 4096, 1, debug={"sketch_path": "sync"}, ctx=c, seen=seen)
    assert m1.path == m2.path == "sync" and m1.sort == ["sort_unique_kernel<true>"]
    assert m2.sort == ["sort_unique_kernel<true>", "sort_unique_kernel<true>"] and m2.sort_branch[0][1].startswith("todo/")


def test_sync_path_large_sets(hg, orc):
    kmers, _ = pool(orc, 40, 34_000)
    rng = np.random.default_rng(13)
    base = np.arange(0, 9000)
    seqs = [dirty(kmers, np.arange(0, 8193)), dirty(kmers, np.arange(10_000, 30_000)),
            dirty(kmers, rng.permutation(np.concatenate([base, base, base[:2000]])))]  # 20 000 raw, 9 000 distinct
    m = run_step(hg, orc, seqs, 40, 4096, 1, debug={"sketch_path": "sync"})
    assert [b[1] for b in m.sort_branch] == ["bucket_lds", "bucket_lds", "bucket_lds"]
    # 4 096 buckets: counted and scattered through global memory
    m = run_step(hg, orc, seqs[:1], 40, 4096, 1, debug={"sort_test_buckets": "4096"})
    assert m.sort_branch[0] == ("bucket_sort_kernel", "bucket_global")
    # 2 buckets of ~10 000 keys: the hash set takes the repeats; with 20 000 distinct keys it gives up -> in place
    m = run_step(hg, orc, seqs[1:], 40, 4096, 0, debug={"sort_test_buckets": "2"})
    assert m.sort_branch[0] == ("sort_unique_kernel<false>", "bucket_lds/gave_up")
    assert m.sort_branch[1] == ("bucket_sort_kernel", "bucket_lds/hashset")
    assert m.sort[-1] == "sort_unique_kernel<false>"


def test_sync_path_slab_split(hg, orc):
    kmers, _ = pool(orc, 40, 34_000)
    rng = np.random.default_rng(14)
    base = np.arange(0, 30_000)
    seqs = [dirty(kmers, np.arange(0, n)) for n in (32767, 32768, 32769)]
    seqs.append(dirty(kmers, rng.permutation(np.concatenate([base, base[:3000]]))))  # 33 000 raw, 30 000 distinct
    for hv_d, layout in ((4096, 1), (1000, 0)):
        m = run_step(hg, orc, seqs, 40, hv_d, layout)
        assert m.path == "sync" and m.encode == ["encode_wave_kernel", "encode_kernel<false>", "encode_kernel<true>",
                                                 "encode_finalize_kernel"]
        assert [b[0] for b in m.encode_branch] == ["encode_kernel<false>", "encode_kernel<false>", "encode_kernel<true>",
                                                   "encode_kernel<false>"]
        assert m.encode_branch[2][1] == "slabs+finalize" and m.encode_branch[3][1] == "block+finalize"


def test_sketch_wraps_the_norm_at_scaled_1(hg, orc):
    rng = np.random.default_rng(15)
    seqs = [rng.choice(ACGT, 600_000)]
    m = run_step(hg, orc, seqs, 1, 4096, 1)
    assert m.path == "sync" and "encode_kernel<true>" in m.encode
    w_hv, _, _ = orc.sketch_genome(seqs[0], K, 1)
    assert int((w_hv.astype(np.int64) ** 2).sum()) > 2**31


# ---- encode reach by batch size -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_genomes", (8191, 8192))
@pytest.mark.parametrize("path", ("sync_free", "sync"))
def test_wave_max_follows_the_batch(hg, orc, n_genomes, path):
    """the wave kernel takes up to 256 hashes below 8 192 genomes and up to 16 368 from there: in a sync-free step of 8 192 the
    eight-wave encoder is not even queued"""
    kmers, _ = pool(orc, 40, 34_000)
    rng = np.random.default_rng(16)
    big = ((600, 16368), (17_000, 16369)) if path == "sync" else ((600, 4000), (17_000, 8000))
    planted = [dirty(kmers, np.arange(a, a + n)) for a, n in ((0, 256), (300, 257)) + big]
    fill = [dirty(kmers, rng.choice(34_000, int(rng.integers(1, 4)), replace=False)) for _ in range(n_genomes - len(planted))]
    seqs = fill[:100] + planted + fill[100:]
    m = run_step(hg, orc, seqs, 40, 1000, 1)
    assert m.path == path
    got = [m.encode_branch[100 + i][0] for i in range(4)]
    if n_genomes >= 8192:
        assert got == ["encode_wave_kernel"] * (3 if path == "sync" else 4) + ["encode_kernel<false>"] * (path == "sync")
        assert m.encode_branch[102][1] == "p14/vec/tail"
        assert m.encode == (["encode_wave_kernel", "sketch_finish_kernel"] if path == "sync_free" else
                            ["encode_wave_kernel", "encode_kernel<false>"])
    else:
        assert got == ["encode_wave_kernel"] + ["encode_kernel<false>"] * 3
        assert "encode_kernel<false>" in m.encode
