"""hg_search_topk* on the device: the k best references per query, selected while blocks of the ANI matrix stream past.
Every comparison is `==`: against the numpy model (tests/search_topk_ref.py) fed with the device's own hg_dist_full_dev
matrix, against the hit-list route (hg_dist_dev + hg_topk_per_query_dev), across block sizes, blocks and shards."""
import os
import subprocess

import numpy as np
import pytest

import search_topk_ref as ref

pytestmark = pytest.mark.gpu

KS = (1, 2, 5, 64)
THS = (0.0, 85.0, 99.5, 100.0, 101.0)
HV_D = 4096


@pytest.fixture(scope="module")
def hg():
    import torch  # noqa: F401  (before the library: see the package's docstring)
    import hypergen_amd
    hypergen_amd.lib()
    return hypergen_amd


@pytest.fixture()
def sctx(hg):
    with hg.Context(0) as c:
        yield c


def norms(hv):
    import torch
    return (hv.to(torch.int64) ** 2).sum(1).to(torch.int32)


def sketches(rows, salt=0, n=900, plant_from=None):
    """clustered i16 HVs (bench.clustered_hvs) + norms on the device; plant_from: every 37th row becomes a copy of a row of
    that set (ANI exactly 100, and ties with the neighbours of the copied row)"""
    import torch
    import bench
    dev = torch.device("cuda:0")
    hv = bench.clustered_hvs(rows, 0, dev, n=n, salt=salt)
    if plant_from is not None:
        for i in range(0, rows, 37):
            hv[i] = plant_from[(i * 7) % plant_from.shape[0]]
    return hv, norms(hv)


def full_matrix(ctx, r, rn, q, qn, ksize=21):
    import torch
    out = torch.empty((r.shape[0], q.shape[0]), dtype=torch.float32, device=r.device)
    torch.cuda.synchronize()
    ctx.dist_full_dev(r.data_ptr(), rn.data_ptr(), r.shape[0], q.data_ptr(), qn.data_ptr(), q.shape[0], HV_D, ksize, out.data_ptr())
    ctx.sync()
    return out.cpu().numpy()


def hits_of(t_out, t_cnt, Q, k):
    return t_out.cpu().numpy().view(np.uint8).view(ref.HIT_DTYPE).reshape(Q, k), t_cnt.cpu().numpy().view(np.uint32)


def search(ctx, r, rn, q, qn, ani_th, k, ksize=21, ref_off=0, qry_off=0, R=None):
    """hg_search_topk_block_dev into buffers pre-filled with 0x5A bytes: every slot and count must be written"""
    import torch
    Q = q.shape[0]
    out = torch.full((Q * k * 3,), 0x5A5A5A5A, dtype=torch.int32, device=q.device)
    cnt = torch.full((Q,), 0x5A5A5A5A, dtype=torch.int32, device=q.device)
    torch.cuda.synchronize()
    ctx.search_topk_dev(r.data_ptr(), rn.data_ptr(), r.shape[0] if R is None else R, q.data_ptr(), qn.data_ptr(), Q, HV_D, ksize,
                        ani_th, k, out.data_ptr(), cnt.data_ptr(), ref_off=ref_off, qry_off=qry_off)
    ctx.sync()
    return hits_of(out, cnt, Q, k)


def assert_same(got, want, what):
    (gh, gc), (wh, wc) = got, want
    assert np.array_equal(gc, wc), (what, np.nonzero(gc != wc)[0][:8])
    if not np.array_equal(gh, wh):
        bad = np.argwhere(gh != wh)[:4]
        raise AssertionError((what, [(tuple(b), gh[tuple(b)], wh[tuple(b)]) for b in bad]))


SHAPES = [(1, 1), (5, 1), (300, 3), (1000, 16), (1000, 17), (2500, 64), (2500, 65), (3000, 700)]
MID = {(300, 3), (1000, 16), (1000, 17), (2500, 64), (2500, 65)}


@pytest.mark.parametrize("R,Q", SHAPES)
def test_search_topk_equals_the_model_on_the_device_matrix(hg, sctx, R, Q):
    """all k x thresholds (and, on the mid shapes, all three metrics) against the model on hg_dist_full_dev's own floats"""
    q, qn = sketches(Q, salt=1)
    r, rn = sketches(R, plant_from=q)
    for metric in ((hg.ANI_MASH, hg.ANI_CONTAINMENT, hg.ANI_MAX_CONTAINMENT) if (R, Q) in MID else (hg.ANI_MASH,)):
        sctx.set_ani_metric(metric)
        ani = full_matrix(sctx, r, rn, q, qn)
        assert ani.min() >= 0.0 and ani.max() == 100.0  # (the planted copies)
        top = ref.topk_sorted(ani, max(KS))
        for k in KS:
            for th in THS:
                assert_same(search(sctx, r, rn, q, qn, th, k), ref.topk_from_sorted(top, th, k), (R, Q, metric, k, th))
    sctx.set_ani_metric(hg.ANI_MASH)


@pytest.fixture(scope="module")
def big(hg):
    """10 000 x 10 000 clustered sketches, their device matrix ordered once for the model"""
    q, qn = sketches(10000, salt=1, n=3333)
    r, rn = sketches(10000, n=3333, plant_from=q)
    with hg.Context(0) as c:
        ani = full_matrix(c, r, rn, q, qn)
    return r, rn, q, qn, ref.topk_sorted(ani, max(KS)), float((ani >= np.float32(85.0)).mean())


def test_search_topk_equals_the_model_at_10000_x_10000(hg, sctx, big):
    r, rn, q, qn, top, dense = big
    assert 0.002 < dense < 0.05  # about 1 % of the pairs pass 85
    for k in KS:
        for th in THS:
            assert_same(search(sctx, r, rn, q, qn, th, k), ref.topk_from_sorted(top, th, k), (k, th))


def test_search_topk_equals_the_hit_list_route_at_10000_x_10000(hg, sctx, big):
    """rows, counts and empty slots of hg_dist_dev(85) + hg_topk_per_query_dev, bit for bit"""
    import torch
    r, rn, q, qn, _, _ = big
    R, Q = r.shape[0], q.shape[0]
    cap = 6_000_000
    d_hits = torch.empty(cap * 3, dtype=torch.int32, device=r.device)
    torch.cuda.synchronize()
    found, st = sctx.dist_dev(r.data_ptr(), rn.data_ptr(), R, q.data_ptr(), qn.data_ptr(), Q, HV_D, 21, False, 85.0, d_hits.data_ptr(), cap)
    assert st == hg.OK and 100_000 < found <= cap
    for k in (1, 3, 64):
        out = torch.full((Q * k * 3,), 0x5A5A5A5A, dtype=torch.int32, device=r.device)
        cnt = torch.full((Q,), 0x5A5A5A5A, dtype=torch.int32, device=r.device)
        torch.cuda.synchronize()
        sctx.topk_per_query_dev(d_hits.data_ptr(), found, Q, k, out.data_ptr(), cnt.data_ptr())
        sctx.sync()
        assert_same(search(sctx, r, rn, q, qn, 85.0, k), hits_of(out, cnt, Q, k), k)


def test_ties_of_identical_references_go_to_the_lowest_indices(hg, sctx):
    """40 copies of one reference row at indices on both sides of block borders (192 rows) and slice borders (32 rows at
    Q = 70, none inside a block at Q = 5): for k < 40 the lowest indices win, in index order"""
    import torch
    for Q in (70, 5):
        q, qn = sketches(Q, salt=1)
        r, rn = sketches(3000)
        at = sorted({31, 32, 33, 63, 64, 190, 191, 192, 193, 383, 384, 385, 575, 576, 1000, 1151, 1152, 1153, 1343, 1344,
                     1535, 1536, 1537, 1900, 1919, 1920, 1921, 2111, 2112, 2303, 2304, 2305, 2500, 2687, 2688, 2879, 2880,
                     2881, 2998, 2999})
        assert len(at) == 40
        r[torch.tensor(at, device=r.device)] = q[2]
        rn = norms(r)
        sctx.set_debug("search_block_rows", 192)
        ani = full_matrix(sctx, r, rn, q, qn)
        assert (ani[at, 2] == 100.0).all() and (ani[:, 2] == 100.0).sum() == 40
        for k in (1, 5, 39):
            h, c = search(sctx, r, rn, q, qn, 99.9, k)
            assert h["ref_idx"][2].tolist() == at[:k] and c[2] == k and (h["ani"][2] == 100.0).all()
            assert_same((h, c), ref.topk_model(ani, 99.9, k), (Q, k))
        sctx.set_debug("search_block_rows", 0)


def test_zero_rows_fill_the_slots_the_positive_anis_leave_in_index_order(hg, sctx):
    """several hundred all-zero reference rows (ANI exactly 0 with every query) at th = 0, k = 64"""
    import torch
    q, qn = sketches(9, salt=1)
    r, rn = sketches(700)
    zero = [i for i in range(700) if i % 100 >= 6]  # 94 of every 100 rows: 658 zero rows, 42 others (fewer than k)
    r[torch.tensor(zero, device=r.device)] = 0
    rn = norms(r)
    for rows in (0, 64):
        sctx.set_debug("search_block_rows", rows)
        ani = full_matrix(sctx, r, rn, q, qn)
        assert (ani[zero] == 0.0).all()
        h, c = search(sctx, r, rn, q, qn, 0.0, 64)
        assert_same((h, c), ref.topk_model(ani, 0.0, 64), rows)
        for j in range(9):
            pos = int((ani[:, j] > 0).sum())
            assert c[j] == 64 and pos < 64
            tail = h[j, pos:]
            # behind the positive ANIs: the rows with ANI 0 in index order (the zero rows, and any other row at exactly 0)
            assert (tail["ani"] == 0.0).all() and tail["ref_idx"].tolist() == np.nonzero(ani[:, j] == 0.0)[0][:64 - pos].tolist()
    sctx.set_debug("search_block_rows", 0)


def test_output_does_not_depend_on_block_rows_blocks_or_shards(hg, sctx):
    import torch
    R, Q, k = 2500, 65, 5
    q, qn = sketches(Q, salt=1)
    r, rn = sketches(R, plant_from=q)
    for th in (0.0, 85.0):
        base = search(sctx, r, rn, q, qn, th, k)
        for rows in (64, 192, 1000, R):
            sctx.set_debug("search_block_rows", rows)
            assert_same(search(sctx, r, rn, q, qn, th, k), base, ("block rows", rows, th))
        sctx.set_debug("search_block_rows", 0)
        # three blocks of reference rows with their offsets, merged on the host
        cuts = [0, 700, 1801, R]
        parts = [search(sctx, r[a:b], rn[a:b], q, qn, th, k, ref_off=a) for a, b in zip(cuts, cuts[1:])]
        assert_same(hg.search_topk_merge([p[0] for p in parts], [p[1] for p in parts], k), base, ("blocks", th))
        # three shards on one device, every shard holding all queries
        with hg.Multi([0, 0, 0]) as m:
            rng = [hg.shard_range(R, s, 3) for s in range(3)]
            rs = [r[a:b].contiguous() for a, b in rng]
            ns = [rn[a:b].contiguous() for a, b in rng]
            torch.cuda.synchronize()
            got = m.search_topk_dev([x.data_ptr() for x in rs], [x.data_ptr() for x in ns], [b - a for a, b in rng],
                                    [q.data_ptr()] * 3, [qn.data_ptr()] * 3, Q, HV_D, 21, th, k)
        assert_same(got, base, ("shards", th))
    # query offsets only relabel
    off = search(sctx, r, rn, q, qn, 85.0, k, ref_off=1000, qry_off=50)
    base = search(sctx, r, rn, q, qn, 85.0, k)
    assert np.array_equal(off[1], base[1])
    live = base[0]["ref_idx"] != ref.EMPTY
    assert np.array_equal(off[0]["ref_idx"][live], base[0]["ref_idx"][live] + 1000)
    assert np.array_equal(off[0]["qry_idx"][live], base[0]["qry_idx"][live] + 50) and np.array_equal(off[0]["ani"], base[0]["ani"])
    # the host-staged form
    host = sctx.search_topk(r.cpu().numpy(), rn.cpu().numpy(), q.cpu().numpy(), qn.cpu().numpy(), 21, 85.0, k)
    assert_same(host, base, "host")


def test_edge_rules(hg, sctx):
    import torch
    L = hg.lib()
    q, qn = sketches(4, salt=1)
    r, rn = sketches(50)
    out = torch.full((4 * 64 * 3,), 0x5A5A5A5A, dtype=torch.int32, device=q.device)
    cnt = torch.full((4,), 0x5A5A5A5A, dtype=torch.int32, device=q.device)
    torch.cuda.synchronize()
    P = lambda t: t.data_ptr()

    def call(R=50, Q=4, k=2, refp=P(r), rnp=P(rn), qp=P(q), qnp=P(qn), outp=P(out), cntp=P(cnt), hv_d=HV_D, ksize=21):
        import ctypes as C
        st = L.hg_search_topk_dev(sctx._h, C.c_void_p(refp), C.c_void_p(rnp), R, C.c_void_p(qp), C.c_void_p(qnp), Q, hv_d, ksize,
                                  C.c_float(0.0), k, C.c_void_p(outp), C.c_void_p(cntp))
        sctx.sync()
        return st

    untouched = lambda: bool((out == 0x5A5A5A5A).all()) and bool((cnt == 0x5A5A5A5A).all())
    # k == 0 or Q == 0: HG_OK, nothing is written (not even with NULL outputs)
    assert call(k=0) == hg.OK and untouched()
    assert call(Q=0) == hg.OK and untouched()
    assert call(k=0, outp=0, cntp=0) == hg.OK
    # k beyond HG_SEARCH_TOPK_MAX
    assert call(k=65) == hg.ERR_UNSUPPORTED and untouched()
    # NULL pointers
    for kw in (dict(refp=0), dict(rnp=0), dict(qp=0), dict(qnp=0), dict(outp=0), dict(cntp=0)):
        assert call(**kw) == hg.ERR_INVALID, kw
    assert L.hg_search_topk_dev(None, None, None, 1, None, None, 1, HV_D, 21, 0, 1, None, None) == hg.ERR_INVALID
    assert untouched()
    # errors of the dist call pass through (its argument checks: HG_ERR_INEXACT has no way to arise from i16 rows)
    assert call(ksize=0) == hg.ERR_INVALID and call(hv_d=0) == hg.ERR_UNSUPPORTED and untouched()
    # R == 0: counts 0, every slot empty (reference pointers may be NULL then)
    assert call(R=0, refp=0, rnp=0, k=64) == hg.OK
    h, c = hits_of(out, cnt, 4, 64)
    assert (c == 0).all() and (h["ref_idx"] == ref.EMPTY).all() and (h["qry_idx"] == ref.EMPTY).all() and (h["ani"] == 0).all()
    # ... and the call works afterwards
    assert_same(search(sctx, r, rn, q, qn, 0.0, 64), ref.topk_model(full_matrix(sctx, r, rn, q, qn), 0.0, 64), "after")
    # the same rules through the multi entry point
    with hg.Multi([0, 0]) as m:
        with pytest.raises(hg.HgError) as e:
            m.search_topk_dev([P(r), P(r)], [P(rn), P(rn)], [25, 25], [P(q)] * 2, [P(qn)] * 2, 4, HV_D, 21, 0.0, 65)
        assert e.value.status == hg.ERR_UNSUPPORTED
        with pytest.raises(hg.HgError) as e:
            m.search_topk_dev([P(r), P(r)], [P(rn), P(rn)], [25, 25], [P(q), 0], [P(qn)] * 2, 4, HV_D, 21, 0.0, 2)
        assert e.value.status == hg.ERR_INVALID
        h, c = m.search_topk_dev([0, 0], [0, 0], [0, 0], [P(q)] * 2, [P(qn)] * 2, 4, HV_D, 21, 0.0, 3)
        assert (c == 0).all() and (h["ref_idx"] == ref.EMPTY).all()


def test_device_memory_stays_within_a_quarter_of_the_full_matrix(hg):
    """R = 60 000, Q = 4 096 in blocks of 4 096 rows on a fresh ctx: free device memory may drop by less than 246 MB across
    the call (a quarter of the 983 MB full matrix; the hit list at th = 0 would be 2.9 GB)"""
    import torch
    dev = torch.device("cuda:0")
    R, Q, k = 60000, 4096, 10
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    r = torch.randint(-40, 41, (R, HV_D), generator=g, device=dev, dtype=torch.int16)
    q = torch.randint(-40, 41, (Q, HV_D), generator=g, device=dev, dtype=torch.int16)
    q[::5] = r[1234:1234 + (Q + 4) // 5]
    rn, qn = norms(r), norms(q)
    out = torch.empty((2, Q * k * 3), dtype=torch.int32, device=dev)
    cnt = torch.empty((2, Q), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    with hg.Context(0) as c:
        c.set_debug("search_block_rows", 4096)
        free0 = torch.cuda.mem_get_info()[0]
        c.search_topk_dev(r.data_ptr(), rn.data_ptr(), R, q.data_ptr(), qn.data_ptr(), Q, HV_D, 21, 0.0, k, out[0].data_ptr(), cnt[0].data_ptr())
        c.sync()
        drop = free0 - torch.cuda.mem_get_info()[0]
    print("free device memory dropped by %.1f MB (limit 246 MB; full matrix %.0f MB)" % (drop / 1e6, R * Q * 4 / 1e6))
    assert drop < 246e6, drop
    with hg.Context(0) as c:  # the automatic block size gives the same rows
        c.search_topk_dev(r.data_ptr(), rn.data_ptr(), R, q.data_ptr(), qn.data_ptr(), Q, HV_D, 21, 0.0, k, out[1].data_ptr(), cnt[1].data_ptr())
        c.sync()
    assert torch.equal(out[0], out[1]) and torch.equal(cnt[0], cnt[1]) and bool((cnt[0] == k).all())
    h, _ = hits_of(out[0], cnt[0], Q, k)
    assert (h["ani"][::5, 0] == 100.0).all() and np.array_equal(h["ref_idx"][::5, 0], 1234 + np.arange((Q + 4) // 5))


def test_cli_search_paths_write_the_same_bytes(hg, tmp_path):
    """--search_path topk, hits and the default: byte-identical TSVs for -n 1 / 3 / 64, -a 80 / 0, one and two shards and
    the containment metric; -n 65 still works (through the hit list)"""
    n = 700
    a, _ = sketches(n)
    b, _ = sketches(n, salt=1)
    a, b = a.cpu().numpy(), b.cpu().numpy()
    a[5] = a[4]
    b[9] = a[4]  # ANI exactly 100 twice for one query: a tie the order must break by reference index
    paths = []
    for name, hv in (("a", a), ("b", b)):
        recs = []
        for i in range(n):
            qb, pk = hg.hv_pack(hv[i])
            recs.append(dict(ksize=21, scaled=1500, canonical=True, seed=123, hv_d=4096, hv_quant_bits=qb,
                             hv_norm_2=int((hv[i].astype(np.int64) ** 2).sum()), file_str="/d/%s/%s%04d.fna" % (name, "x" * (i % 3), i),
                             hv=pk.view(np.int16)))
        p = str(tmp_path / (name + ".sketch"))
        hg.write_sketch_file(p, recs)
        paths.append(p)
    env = dict(os.environ, RUST_LOG="debug")

    def run(extra):
        tsv = str(tmp_path / "s.tsv")
        if os.path.exists(tsv):
            os.remove(tsv)
        res = subprocess.run([hg.CLI_PATH, "search", "-r", paths[0], "-q", paths[1], "-o", tsv] + extra, capture_output=True, text=True, env=env)
        assert res.returncode == 0, (extra, res.stderr)
        return open(tsv, "rb").read(), "selected block by block" in res.stdout

    cases = [["-n", str(k), "-a", th, "--shards", sh] for k in (1, 3, 64) for th in ("80", "0") for sh in ("1", "2")]
    cases += [["-n", "3", "-a", "80", "--shards", sh, "--ani_metric", "containment"] for sh in ("1", "2")]
    for case in cases:
        (hits, f_hits), (topk, f_topk), (auto, f_auto) = (run(case + ["--search_path", "hits"]), run(case + ["--search_path", "topk"]),
                                                           run(case))
        assert not f_hits and f_topk and f_auto, case  # the default takes the fused path up to -n 64
        assert hits == topk == auto, case
        lines = hits.count(b"\n")
        assert lines >= n if case[3] == "80" else lines == n * int(case[1]), (case, lines)
    (hits, f_hits), (auto, f_auto) = run(["-n", "65", "-a", "80", "--search_path", "hits"]), run(["-n", "65", "-a", "80"])
    assert hits == auto and not f_hits and not f_auto and hits.count(b"\n") > n
    bad = subprocess.run([hg.CLI_PATH, "search", "-r", paths[0], "-q", paths[1], "-o", str(tmp_path / "x.tsv"), "-n", "65", "--search_path", "topk"],
                         capture_output=True, text=True)
    assert bad.returncode == 2 and "search_path" in bad.stderr
