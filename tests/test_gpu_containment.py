"""The containment ANI metrics on the device (hg_ctx_set_ani_metric): every path that turns a dot product into an ANI, EQUAL
to tests/containment_ref.py bit for bit -- full matrices, hit sets with their values, every operand path, the pre-filter
under hit densities the Mash-style bound would cut, the small-side kernel, blocks and shards, clustering, and what the
metric is for: the identity of a genome fragment."""
import os
import subprocess

import numpy as np
import pytest
import torch

import containment_ref as cr

pytestmark = pytest.mark.gpu
METRICS = (cr.MASH, cr.CONTAINMENT, cr.MAX_CONTAINMENT)


@pytest.fixture(scope="module")
def hg():
    import hypergen_amd
    return hypergen_amd


@pytest.fixture(scope="module")
def ctx(hg):
    c = hg.Context(0)
    c.set_stream(torch.cuda.current_stream().cuda_stream)
    yield c
    c.close()


@pytest.fixture
def metric_ctx(ctx):
    """the module's ctx, back on the default metric and paths after each test"""
    yield ctx
    ctx.set_ani_metric(cr.MASH)
    ctx.set_debug("dist_path", "")
    ctx.set_debug("pair_limit", "0")
    ctx.set_debug("cluster_hit_cap", "0")


@pytest.fixture(scope="module")
def frag():
    hv, n2, _ = cr.fragment_hvs(384, seed=5)
    return hv, n2, cr.exact_dots(hv, hv)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and bool((a.view(np.uint32) == b.view(np.uint32)).all())


def hit_dict(h):
    return {(int(r), int(q)): np.float32(a) for r, q, a in zip(h["ref_idx"], h["qry_idx"], h["ani"])}


def want_hits(ani, th, symmetric=False, r_off=0, q_off=0):
    m = ani >= np.float32(th)
    if symmetric:
        m &= np.triu(np.ones_like(m), 1)
    i, j = np.nonzero(m)
    return {(int(a) + r_off, int(b) + q_off): ani[a, b] for a, b in zip(i, j)}


def assert_same_hits_np(got, ani, th):
    """the same check for large matrices, vectorised: got equals {(i, j): ani[i, j] >= th}"""
    i, j = np.nonzero(ani >= np.float32(th))
    key = np.sort(got["ref_idx"].astype(np.int64) * ani.shape[1] + got["qry_idx"].astype(np.int64))
    assert key.size == i.size and (key == i.astype(np.int64) * ani.shape[1] + j).all()
    assert (got["ani"].view(np.uint32) == ani[got["ref_idx"], got["qry_idx"]].view(np.uint32)).all()


def fmt3(a):
    """the CLI's "{:.3}" of a float32 ANI (hg_cli.cpp: put_ani)"""
    v = int(np.rint(float(min(max(float(a), 0.0), 100.0)) * 1000.0))
    return "%d.%03d" % (v // 1000, v % 1000)


def assert_same_hits(got, want):
    g = hit_dict(got)
    assert len(g) == len(got), "duplicate hits"
    assert g.keys() == want.keys(), (len(g), len(want))
    bad = [k for k in g if np.float32(g[k]).view(np.uint32) != np.float32(want[k]).view(np.uint32)]
    assert not bad, bad[:5]


# ---- 1. the formula on its own ---------------------------------------------------------------------------------------
def test_fresh_ctx_reports_mash_and_rejects_unknown(hg):
    with hg.Context(0) as c:
        assert c.ani_metric() == cr.MASH
        for bad in (-1, 3, 100):
            with pytest.raises(hg.HgError):
                c.set_ani_metric(bad)
        assert c.ani_metric() == cr.MASH
        c.set_ani_metric(cr.MAX_CONTAINMENT)
        assert c.ani_metric() == cr.MAX_CONTAINMENT


@pytest.mark.parametrize("metric", METRICS)
def test_ani_from_dots_dev(metric_ctx, orc, metric):
    ctx = metric_ctx
    rng = np.random.default_rng(metric)
    n = 200_000
    nr = rng.integers(0, 1 << 27, n).astype(np.int32)
    nq = rng.integers(0, 1 << 27, n).astype(np.int32)
    dot = (np.minimum(nr, nq) * rng.uniform(-0.1, 1.2, n)).astype(np.int32)
    edge = np.array([[0, 100, 100], [-1, 100, 100], [-(1 << 30), 5, 7], [0, 0, 0], [5, 0, 0], [5, 3, 0], [5, 0, 3],
                     [200, 100, 100], [100, 50, 100], [100, 100, 50], [1 << 30, 1 << 30, (1 << 30) + 1],
                     [(1 << 29) + 1, 1 << 30, 1 << 29], [2147483647, 2147483647, 2147483647], [1, 2147483647, -2147483648],
                     [-2147483648, -2147483648, 2147483647], [7, -3, 9], [7, 9, -3], [1000, 2000, 1000]], np.int64)
    dot = np.concatenate([dot, edge[:, 0].astype(np.int32)])
    nr = np.concatenate([nr, edge[:, 1].astype(np.int32)])
    nq = np.concatenate([nq, edge[:, 2].astype(np.int32)])
    d = [torch.from_numpy(v).cuda() for v in (dot, nr, nq)]
    out = torch.empty(dot.size, dtype=torch.float32, device="cuda:0")
    ctx.set_ani_metric(metric)
    for k in (1, 21, 32, 64, 255):
        ctx.ani_from_dots_dev(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), dot.size, k, out.data_ptr())
        ctx.sync()
        assert same_bits(out.cpu().numpy(), cr.ani_ref(orc, dot, nr, nq, k, metric)), k


# ---- 2. full matrices and thresholded hit sets on every operand path ------------------------------------------------
@pytest.mark.parametrize("path", ["", "i8", "f16", "cen"])
@pytest.mark.parametrize("metric", METRICS)
def test_full_and_thresholded_on_fragments(metric_ctx, hg, orc, frag, metric, path):
    ctx = metric_ctx
    hv, n2, dots = frag
    want = cr.ani_ref(orc, dots, n2[:, None], n2[None, :], 21, metric)
    if metric == cr.MASH:
        assert same_bits(want, orc.ani_matrix(hv, n2, hv, n2, 21))
    ctx.set_ani_metric(metric)
    ctx.set_debug("dist_path", path)
    assert same_bits(ctx.dist_full(hv, n2, hv, n2, 21), want)
    q = hv[::-1].copy()  # (a second set: the same rows in reverse order)
    qn = n2[::-1].copy()
    want_rq = want[:, ::-1]
    assert same_bits(ctx.dist_full(hv, n2, q, qn, 21), want_rq)
    vals = np.sort(want[want > 50].ravel())
    for th in (85.0, 95.0, float(vals[len(vals) // 2])):  # the last: a value of the matrix, hits exactly at it
        assert_same_hits(ctx.dist(hv, n2, q, qn, 21, False, th), want_hits(want_rq, th))
        if metric == cr.CONTAINMENT:
            with pytest.raises(hg.HgError) as e:
                ctx.dist(hv, n2, hv, n2, 21, True, th)
            assert e.value.status == hg.ERR_INVALID
        else:
            assert_same_hits(ctx.dist(hv, n2, hv, n2, 21, True, th), want_hits(want, th, symmetric=True))
    assert len(want_hits(want, 95.0)) > 1000


@pytest.mark.parametrize("metric", METRICS)
def test_integer_fallback(metric_ctx, orc, frag, metric):
    ctx = metric_ctx
    hv, n2, _ = frag
    hv = hv[:100].copy()
    hv[:, 7] = np.where(np.arange(100) % 2 == 0, 3000, -3001).astype(np.int16)  # |x| > 2048: no f16 operand path
    n2 = cr.norms(hv)
    want = cr.ani_ref(orc, cr.exact_dots(hv, hv), n2[:, None], n2[None, :], 21, metric)
    ctx.set_ani_metric(metric)
    ctx.set_debug("dist_path", "f16")
    for th in (85.0, 95.0):
        assert_same_hits(ctx.dist(hv, n2, hv[::-1].copy(), n2[::-1].copy(), 21, False, th), want_hits(want[:, ::-1], th))
        assert ctx.last_dist_path() == 2
    assert same_bits(ctx.dist_full(hv, n2, hv, n2, 21), want)


# ---- 3. the pre-filter where the Mash-style bound would lose the hits ------------------------------------------------
@pytest.fixture(scope="module")
def stress():
    r, rn, q, qn = cr.stress_hvs(4096, 4096)
    return r, rn, q, qn, cr.exact_dots(r, q)


@pytest.mark.parametrize("metric", [cr.CONTAINMENT, cr.MAX_CONTAINMENT])
def test_prefilter_dense_containment(metric_ctx, orc, stress, metric):
    ctx = metric_ctx
    r, rn, q, qn, dots = stress
    want = cr.ani_ref(orc, dots, rn[:, None], qn[None, :], 21, metric)
    mash = cr.ani_ref(orc, dots, rn[:, None], qn[None, :], 21, cr.MASH)
    assert (want >= 95.0).mean() > 0.9 and (mash >= 95.0).mean() < 0.01
    ctx.set_ani_metric(metric)
    got = ctx.dist(r, rn, q, qn, 21, False, 95.0, cap=want.size + 1024)
    assert ctx.last_dist_path() in (1, 3)  # (> 256^3 pairs: byte or centred operands by default)
    assert_same_hits_np(got, want, 95.0)


# ---- 4. the small-side streaming kernel, both directions ------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
def test_small_side_kernel(metric_ctx, orc, frag, metric):
    ctx = metric_ctx
    hv, n2, dots = frag
    want = cr.ani_ref(orc, dots, n2[:, None], n2[None, :], 21, metric)
    ctx.set_ani_metric(metric)
    d_hv = torch.from_numpy(hv).cuda()
    d_n2 = torch.from_numpy(n2).cuda()
    out = torch.empty(3 * 10000, dtype=torch.int32, device="cuda:0")
    for small, in_rows in ((5, True), (16, True), (1, False), (16, False)):
        R, Q = (small, 384) if in_rows else (384, small)
        found, st = ctx.dist_dev(d_hv.data_ptr(), d_n2.data_ptr(), R, d_hv[-Q:].data_ptr(), d_n2[-Q:].data_ptr(), Q, 4096, 21,
                                 False, 85.0, out.data_ptr(), 10000)
        assert st == 0 and ctx.last_kernel("dist") == ("dist_skinny_kernel<true>" if in_rows else "dist_skinny_kernel<false>")
        h = out[: 3 * found].cpu().numpy().view(np.uint32).reshape(-1, 3)
        got = np.zeros(found, hg_dtype())
        got["ref_idx"], got["qry_idx"], got["ani"] = h[:, 0], h[:, 1], h[:, 2].view(np.float32)
        assert_same_hits(got, want_hits(want[:R, 384 - Q:], 85.0))


def hg_dtype():
    import hypergen_amd
    return hypergen_amd.ANI_HIT_DTYPE


# ---- 5. blocks, prepared operands, shards ---------------------------------------------------------------------------
def dev_hits(ctx, fn, cap=1 << 20):
    out = torch.empty(3 * cap, dtype=torch.int32, device="cuda:0")
    found, st = fn(out.data_ptr(), cap)
    assert st == 0
    h = out[: 3 * found].cpu().numpy().view(np.uint32).reshape(-1, 3)
    got = np.zeros(found, hg_dtype())
    got["ref_idx"], got["qry_idx"], got["ani"] = h[:, 0], h[:, 1], h[:, 2].view(np.float32)
    return got


@pytest.mark.parametrize("metric", METRICS)
def test_blocks_and_prepared_operands(metric_ctx, orc, frag, metric):
    ctx = metric_ctx
    hv, n2, dots = frag
    want = cr.ani_ref(orc, dots, n2[:, None], n2[None, :], 21, metric)
    ctx.set_ani_metric(metric)
    d_hv, d_n2 = torch.from_numpy(hv).cuda(), torch.from_numpy(n2).cuda()
    th = 90.0
    # row blocks of one comparison at their global offsets: the union is the one-call result
    union = {}
    for r0 in range(0, 384, 100):
        rows = min(100, 384 - r0)
        got = dev_hits(ctx, lambda o, c: ctx.dist_block_dev(d_hv[r0:].data_ptr(), d_n2[r0:].data_ptr(), rows, r0, d_hv.data_ptr(),
                                                             d_n2.data_ptr(), 384, 0, 4096, 21, False, th, o, c))
        union.update(hit_dict(got))
    one = dev_hits(ctx, lambda o, c: ctx.dist_dev(d_hv.data_ptr(), d_n2.data_ptr(), 384, d_hv.data_ptr(), d_n2.data_ptr(), 384, 4096,
                                                  21, False, th, o, c))
    assert_same_hits(one, want_hits(want, th))
    assert union.keys() == hit_dict(one).keys() and all(union[k] == v for k, v in hit_dict(one).items())
    # prepared reference operands
    import hypergen_amd as hg
    rows_p = hg.lib().hg_dist_ops_padded_rows(384)
    ops = torch.zeros(rows_p * hg.lib().hg_dist_ops_row_bytes(4096), dtype=torch.uint8, device="cuda:0")
    meta = torch.zeros(384 * hg.lib().hg_dist_ops_meta_bytes(), dtype=torch.uint8, device="cuda:0")
    flag = torch.zeros(1, dtype=torch.int32, device="cuda:0")
    ctx.dist_prep_ops_dev(d_hv.data_ptr(), 384, 4096, ops.data_ptr(), meta.data_ptr(), flag.data_ptr())
    got = dev_hits(ctx, lambda o, c: ctx.dist_block_ops_dev(ops.data_ptr(), meta.data_ptr(), d_n2.data_ptr(), 384, 0, None,
                                                            flag.data_ptr(), 1, d_hv.data_ptr(), d_n2.data_ptr(), 384, 0, 4096, 21,
                                                            False, th, o, c))
    assert_same_hits(got, want_hits(want, th))


@pytest.mark.parametrize("metric", METRICS)
def test_two_shards_on_one_gpu(hg, orc, frag, metric):
    hv, n2, dots = frag
    want = cr.ani_ref(orc, dots, n2[:, None], n2[None, :], 21, metric)
    with hg.Multi([0, 0]) as m:
        m.set_ani_metric(metric)
        assert all(hg.lib().hg_ctx_ani_metric(m.ctx_handle(s)) == metric for s in range(2))
        assert_same_hits(m.dist(hv, n2, hv, n2, 21, False, 90.0), want_hits(want, 90.0))
        d = [torch.from_numpy(x).cuda() for x in (hv[:200], n2[:200], hv[200:], n2[200:])]
        got = m.dist_dev([d[0].data_ptr(), d[2].data_ptr()], [d[1].data_ptr(), d[3].data_ptr()], [200, 184], None, None, None, 4096,
                         21, metric != cr.CONTAINMENT, 90.0)
        assert_same_hits(got, want_hits(want, 90.0, symmetric=metric != cr.CONTAINMENT))
        if metric == cr.CONTAINMENT:
            with pytest.raises(hg.HgError):
                m.dist(hv, n2, hv, n2, 21, True, 90.0)


def test_more_than_2_32_pairs_max_containment(metric_ctx, hg):
    """one hg_dist_dev call of 66 000 x 66 000 pairs (> 2^32, row blocks inside the call) equals the same comparison run
    as explicit blocks of reference rows"""
    import bench
    ctx = metric_ctx
    n = 66_000
    hv = bench.clustered_hvs(n, 0, "cuda:0")
    n2 = (hv.int() ** 2).sum(1).int()
    ctx.set_ani_metric(cr.MAX_CONTAINMENT)
    torch.cuda.synchronize()
    whole = dev_hits(ctx, lambda o, c: ctx.dist_dev(hv.data_ptr(), n2.data_ptr(), n, hv.data_ptr(), n2.data_ptr(), n, 4096, 21,
                                                    False, 95.0, o, c), cap=8_000_000)
    assert len(whole) > 1_000_000
    parts = {}
    for r0 in range(0, n, 16_500):
        got = dev_hits(ctx, lambda o, c: ctx.dist_block_dev(hv[r0:].data_ptr(), n2[r0:].data_ptr(), 16_500, r0, hv.data_ptr(),
                                                             n2.data_ptr(), n, 0, 4096, 21, False, 95.0, o, c), cap=4_000_000)
        parts.update(hit_dict(got))
    w = hit_dict(whole)
    assert w.keys() == parts.keys() and all(parts[k] == v for k, v in w.items())


# ---- 6. switching back ----------------------------------------------------------------------------------------------
def test_switching_back_to_mash(metric_ctx, orc, frag):
    ctx = metric_ctx
    hv, n2, _ = frag
    ctx.set_ani_metric(cr.CONTAINMENT)
    c1 = ctx.dist_full(hv, n2, hv, n2, 21)
    ctx.set_ani_metric(cr.MASH)
    assert ctx.ani_metric() == cr.MASH
    want = orc.ani_matrix(hv, n2, hv, n2, 21)
    assert same_bits(ctx.dist_full(hv, n2, hv, n2, 21), want) and not same_bits(c1, want)
    assert_same_hits(ctx.dist(hv, n2, hv, n2, 21, True, 90.0), want_hits(want, 90.0, symmetric=True))


# ---- 7. clustering under max containment ----------------------------------------------------------------------------
def components(n, i, j):
    parent = np.arange(n)

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for a, b in zip(i, j):
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    rep = np.array([find(x) for x in range(n)], np.uint32)
    ids = {r: k for k, r in enumerate(sorted(set(rep.tolist())))}
    return rep, np.array([ids[r] for r in rep], np.uint32), len(ids)


def test_cluster_max_containment(metric_ctx, hg, orc, frag):
    ctx = metric_ctx
    hv, n2, dots = frag
    want = cr.ani_ref(orc, dots, n2[:, None], n2[None, :], 21, cr.MAX_CONTAINMENT)
    ctx.set_ani_metric(cr.MAX_CONTAINMENT)
    for th in (90.0, 95.0, 99.0):
        i, j = np.nonzero(np.triu(want >= np.float32(th), 1))
        rep, cl, nc = components(384, i, j)
        for cap in ("0", "50"):
            ctx.set_debug("cluster_hit_cap", cap)
            got = ctx.cluster(hv, n2, 21, th)
            assert (got[0] == rep).all() and (got[1] == cl).all() and got[2] == nc, (th, cap)
    ctx.set_ani_metric(cr.CONTAINMENT)
    with pytest.raises(hg.HgError) as e:
        ctx.cluster(hv, n2, 21, 95.0)
    assert e.value.status == hg.ERR_INVALID


# ---- 8. what the metric is for ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def genomes():
    g = cr.synth(2024, 3_000_000)
    m = cr.mutate(g, 0.02, 7)
    return g, m, cr.fragment(m, 0.30, 3)


def test_fragment_identity(metric_ctx, hg, genomes):
    ctx = metric_ctx
    g, m, f = genomes
    hv, n2, _ = ctx.sketch_batch([b"N" + s for s in (g, m, f)], hg.default_params(scaled=300))
    ctx.set_ani_metric(cr.CONTAINMENT)
    cont = ctx.dist_full(hv[:1], n2[:1], hv[2:], n2[2:], 21)[0, 0]  # the fragment (query) in the original (reference)
    ctx.set_ani_metric(cr.MASH)
    mash = ctx.dist_full(hv[:1], n2[:1], hv[2:], n2[2:], 21)[0, 0]
    mash_full = ctx.dist_full(hv[:1], n2[:1], hv[1:2], n2[1:2], 21)[0, 0]
    ctx.set_ani_metric(cr.MAX_CONTAINMENT)
    maxc_full = ctx.dist_full(hv[:1], n2[:1], hv[1:2], n2[1:2], 21)[0, 0]
    assert 97.3 <= cont <= 98.7, cont
    assert mash < 96.0, mash
    assert abs(maxc_full - mash_full) <= 0.1, (maxc_full, mash_full)


# ---- 9. the command line end to end ---------------------------------------------------------------------------------
def test_cli_end_to_end(hg, orc, tmp_path):
    d_ref, d_qry = tmp_path / "ref", tmp_path / "qry"
    d_ref.mkdir(), d_qry.mkdir()
    bases = [cr.synth(100 + i, 400_000) for i in range(3)]
    for i, b in enumerate(bases):
        cr.write_fasta(str(d_ref / ("g%d.fna" % i)), b, "g%d" % i)
        mut = cr.mutate(b, 0.01, 10 + i)
        for frac in (0.2, 0.5, 0.8):
            cr.write_fasta(str(d_qry / ("g%d_f%02d.fna" % (i, int(frac * 100)))), cr.fragment(mut, frac, i), "f")
    sk_r, sk_q = str(tmp_path / "r.sketch"), str(tmp_path / "q.sketch")
    for d, sk in ((d_ref, sk_r), (d_qry, sk_q)):
        r = subprocess.run([hg.CLI_PATH, "sketch", "-p", str(d), "-o", sk, "-s", "200", "-t", "4"], capture_output=True, text=True,
                           timeout=300)
        assert r.returncode == 0, r.stderr
    R, Q = hg.read_sketch_file(sk_r), hg.read_sketch_file(sk_q)

    def rows(recs):  # the .sketch contents: decompressed HVs and the stored norms
        hv = np.stack([hg.hv_unpack(x["hv"].view(np.uint8), x["hv_d"], x["hv_quant_bits"]) for x in recs])
        return hv, cr.wrap_i32([x["hv_norm_2"] for x in recs])

    def tsv(rr, qq, ani, th, drop_diag):
        """dump_ani_file's order: a stable ascending sort by ANI over the row-major enumeration, reversed"""
        hits = [(ani[i, j], i, j) for i in range(ani.shape[0]) for j in range(ani.shape[1])
                if ani[i, j] >= np.float32(th) and not (drop_diag and i == j)]
        hits.sort(key=lambda t: (t[0], t[1] * ani.shape[1] + t[2]))
        hits.reverse()
        return "".join("%s\t%s\t%s\n" % (rr[i]["file_str"], qq[j]["file_str"], fmt3(a)) for a, i, j in hits)

    hr, nr = rows(R)
    hq, nq = rows(Q)
    ani_rq = cr.ani_ref(orc, cr.exact_dots(hr, hq), nr[:, None], nq[None, :], 21, cr.CONTAINMENT)
    out = str(tmp_path / "c.tsv")
    r = subprocess.run([hg.CLI_PATH, "dist", "-r", sk_r, "-q", sk_q, "-o", out, "-a", "90", "--ani_metric", "containment"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert open(out).read() == tsv(R, Q, ani_rq, 90.0, False)
    assert open(out).read().count("\n") >= 9  # every fragment in its parent
    # one file on both sides: every ordered pair i != j
    ani_qq = cr.ani_ref(orc, cr.exact_dots(hq, hq), nq[:, None], nq[None, :], 21, cr.CONTAINMENT)
    r = subprocess.run([hg.CLI_PATH, "dist", "-r", sk_q, "-q", sk_q, "-o", out, "-a", "90", "--ani_metric", "containment"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert open(out).read() == tsv(Q, Q, ani_qq, 90.0, True)
    # search: the references that contain each query best
    r = subprocess.run([hg.CLI_PATH, "search", "-r", sk_r, "-q", sk_q, "-o", out, "-n", "2", "-a", "50", "--ani_metric",
                        "containment"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    best = {}
    for line in open(out).read().splitlines():
        qf, rf, _ = line.split("\t")
        best.setdefault(qf, rf)
    for x in Q:
        g = os.path.basename(x["file_str"]).split("_")[0]
        assert os.path.basename(best[x["file_str"]]) == g + ".fna"
    # cluster: each fragment with its parent genome under max containment
    both = str(tmp_path / "all.sketch")
    d_all = tmp_path / "all"
    d_all.mkdir()
    for p in list(d_ref.iterdir()) + list(d_qry.iterdir()):
        os.symlink(p, d_all / p.name)
    r = subprocess.run([hg.CLI_PATH, "sketch", "-p", str(d_all), "-o", both, "-s", "200", "-t", "4"], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([hg.CLI_PATH, "cluster", "-p", both, "-o", out, "-a", "95", "--ani_metric", "max_containment"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    cl = {}
    for line in open(out).read().splitlines():
        f, c, _ = line.split("\t")
        cl[os.path.basename(f)] = c
    for i in range(3):
        assert len({c for f, c in cl.items() if f.startswith("g%d" % i)}) == 1
    assert len(set(cl.values())) == 3
