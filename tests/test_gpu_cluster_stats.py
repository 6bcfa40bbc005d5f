"""Cluster statistics on the device (hg_cluster_stats*, `hyper-gen cluster --stats`): every field of the node records and of
the cluster records EQUAL to the model of tests/cluster_stats_ref.py -- the matrix form at the edges of the 16-byte loads
and of the 256-lane scan (rows that start misaligned: n % 4 != 0), with interleaved assignments, one cluster, singletons and
ids without members, ties everywhere, values outside [0, 100], garbage on the diagonal, an asymmetric matrix, each output
absent in turn and the argument faults; resident sketches against the oracle's matrix under both symmetric metrics and
against hg_dist_full_dev's matrix in blocks of several heights, on a borrowed stream and through the host form; the
chaining of single linkage read off the statistics; and end to end through the command line."""
import os
import subprocess
import sys

import numpy as np
import pytest

import cluster_average_ref as av
import cluster_stats_ref as st
import containment_ref as cr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gctx():
    import torch
    import hypergen_amd as hg
    with hg.Context(0) as c:
        yield c, hg, torch.device("cuda:0")


@pytest.fixture(autouse=True)
def clean_hooks(gctx):
    yield
    c = gctx[0]
    c.set_debug("stats_block_rows", "0")
    c.set_ani_metric(cr.MASH)


def records(t, count, dtype):
    return t.cpu().numpy()[:count * dtype.itemsize].view(dtype).copy()


def out_buffers(dev, n, k):
    """device bytes for n node records and k cluster records, filled with a pattern no result has"""
    import torch
    return (torch.full((max(n, 1) * 24,), 0xAB, dtype=torch.uint8, device=dev),
            torch.full((max(k, 1) * 48,), 0xAB, dtype=torch.uint8, device=dev))


def run_matrix(gctx, a, cl, k, want=("node", "stat"), shift=0):
    """hg_cluster_stats_matrix_dev -> (node records or None, cluster records or None); shift: the matrix and the ids start
    that many elements behind a 16-byte boundary"""
    import torch
    c, hg, dev = gctx
    n = a.shape[0]
    d = torch.zeros(n * n + shift + 4, dtype=torch.float32, device=dev)
    d[shift:shift + n * n] = torch.from_numpy(np.ascontiguousarray(a, np.float32).reshape(-1)).to(dev)
    d_cl = torch.zeros(n + shift + 4, dtype=torch.int32, device=dev)
    d_cl[shift:shift + n] = torch.from_numpy(np.asarray(cl, np.uint32).view(np.int32)).to(dev)
    d_node, d_stat = out_buffers(dev, n, k)
    torch.cuda.synchronize()  # (the ctx runs on its own stream)
    c.cluster_stats_matrix_dev(d.data_ptr() + 4 * shift, n, d_cl.data_ptr() + 4 * shift, k,
                               d_node.data_ptr() if "node" in want else None, d_stat.data_ptr() if "stat" in want else None)
    if "node" not in want:
        assert (d_node.cpu().numpy() == 0xAB).all()
    if "stat" not in want:
        assert (d_stat.cpu().numpy() == 0xAB).all()
    return (records(d_node, n, st.NODE_DTYPE) if "node" in want else None, records(d_stat, k, st.CLUSTER_DTYPE) if "stat" in want else None)


def assert_same(got, want):
    for g, w, what in zip(got, want, ("node", "cluster")):
        if g is None:
            continue
        assert g.dtype == w.dtype and g.shape == w.shape, what
        for name in w.dtype.names:
            bad = np.flatnonzero(g[name] != w[name])
            assert bad.size == 0, "%s records: %s differs at %s: %s != %s" % (what, name, bad[:5], g[name][bad[:5]], w[name][bad[:5]])


def against_model(gctx, a, cl, k, **kw):
    want = st.stats_model(a, cl, k)
    got = run_matrix(gctx, a, cl, k, **kw)
    assert_same(got, want)
    return got


def interleaved(n, k, rng):
    """ids 0 .. k - 1 dealt round the items, then some swapped about: non-contiguous, every id used when n >= k"""
    cl = np.arange(n) % k
    swap = rng.permutation(n)[: n // 3]
    cl[swap] = cl[swap[::-1]]
    return cl.astype(np.uint32)


# ---- the matrix form ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3])
def test_tiny(gctx, n):
    rng = np.random.default_rng(n)
    a = rng.uniform(70.0, 100.0, (n, n)).astype(np.float32)
    for cl in ([0] * n, list(range(n)), [0, 1, 0][:n]):
        for shift in (0, 1, 2, 3):
            against_model(gctx, a, cl, max(cl) + 1, shift=shift)
    if n == 3:
        a = np.array([[0, 96, 0], [96, 0, 96], [0, 96, 0]], np.float32)
        node, stat = against_model(gctx, a, [0, 0, 0], 1)
        assert (stat["within_min"][0], stat["medoid"][0], stat["within_min_a"][0], stat["within_min_b"][0]) == (0, 1, 0, 2)


@pytest.mark.parametrize("n", [255, 256, 257, 1023, 1024, 1025])
def test_edges_of_the_row_scan(gctx, n):
    """n % 4 != 0: three rows in four start off a 16-byte boundary; 1023 .. 1025: one step of the 256-lane scan and its edge"""
    rng = np.random.default_rng(n)
    a = rng.uniform(60.0, 100.0, (n, n)).astype(np.float32)
    cl = interleaved(n, 7, rng)
    node, stat = against_model(gctx, a, cl, 7)
    assert (stat["size"] > 1).all() and (node["within_min_idx"] != st.NONE).all()
    if n in (256, 257):
        for shift in (1, 2, 3):  # (the ids behind the head aligned while the row is not, and the other way round)
            against_model(gctx, a, cl, 7, shift=shift)


def test_assignments(gctx):
    rng = np.random.default_rng(21)
    n = 130
    a = rng.uniform(60.0, 100.0, (n, n)).astype(np.float32)
    node, stat = against_model(gctx, a, np.zeros(n, np.uint32), 1)  # one cluster: nothing outside
    assert (node["outside_max_idx"] == st.NONE).all() and stat["outside_idx"][0] == st.NONE and stat["size"][0] == n
    node, stat = against_model(gctx, a, np.arange(n, dtype=np.uint32)[::-1].copy(), n)  # all singletons, ids descending
    assert (node["within_min"] == st.NONE).all() and (stat["medoid"] == np.arange(n)[::-1]).all()
    cl = (interleaved(n, 5, rng) * 3 + 2).astype(np.uint32)  # ids 2, 5, .. 14 of 40: most ids have no members
    node, stat = against_model(gctx, a, cl, 40)
    assert (stat["size"] == 0).sum() == 35 and (stat["first"][stat["size"] == 0] == st.NONE).all()


def test_values(gctx):
    rng = np.random.default_rng(22)
    n = 203
    cl = interleaved(n, 6, rng)
    ties = (rng.integers(0, 4, (n, n)) * 25.0).astype(np.float32)  # ties everywhere: every argmin and argmax is decided by index
    against_model(gctx, ties, cl, 6)
    against_model(gctx, np.full((n, n), 97.0, np.float32), cl, 6)
    a = rng.uniform(60.0, 100.0, (n, n)).astype(np.float32)  # (not symmetric: every row has its own values)
    assert not np.array_equal(a, a.T)
    want = against_model(gctx, a, cl, 6)
    assert_same(run_matrix(gctx, a.T.copy(), cl, 6), st.stats_model(a.T, cl, 6))
    # values outside [0, 100] count as dist would print them; the diagonal is not looked at
    b = a.copy()
    b[0, 1], b[1, 0], b[2, 9], b[9, 2], b[3, 4], b[4, 3], b[5, 7], b[7, 5] = np.nan, np.inf, 250.0, -np.inf, -7.0, np.nan, np.inf, 250.0
    against_model(gctx, b, cl, 6)
    g = a.copy()
    g[np.arange(n), np.arange(n)] = rng.uniform(-1e30, 1e30, n).astype(np.float32)
    g[7, 7], g[8, 8], g[9, 9] = np.nan, np.inf, -np.inf
    assert_same(run_matrix(gctx, g, cl, 6), want)


def test_each_output_may_be_absent_but_not_both(gctx):
    import torch
    c, hg, dev = gctx
    rng = np.random.default_rng(23)
    n = 77
    a = rng.uniform(60.0, 100.0, (n, n)).astype(np.float32)
    cl = interleaved(n, 4, rng)
    want = st.stats_model(a, cl, 4)
    assert_same(run_matrix(gctx, a, cl, 4, want=("node",)), want)
    assert_same(run_matrix(gctx, a, cl, 4, want=("stat",)), want)
    with pytest.raises(hg.HgError) as e:
        run_matrix(gctx, a, cl, 4, want=())
    assert e.value.status == hg.ERR_INVALID
    d = torch.zeros(n * n, dtype=torch.float32, device=dev)
    d_node, d_stat = out_buffers(dev, n, 4)
    with pytest.raises(hg.HgError) as e:
        c.cluster_stats_matrix_dev(d.data_ptr(), n, None, 4, d_node.data_ptr(), d_stat.data_ptr())
    assert e.value.status == hg.ERR_INVALID
    with pytest.raises(hg.HgError) as e:
        c.cluster_stats_matrix_dev(d.data_ptr(), 1 << 31, d.data_ptr(), 4, d_node.data_ptr(), d_stat.data_ptr())
    assert e.value.status == hg.ERR_UNSUPPORTED
    against_model(gctx, a, cl, 4)


def test_an_id_beyond_n_clusters_is_invalid_and_the_next_call_starts_clean(gctx):
    c, hg, dev = gctx
    rng = np.random.default_rng(24)
    n = 300
    a = rng.uniform(60.0, 100.0, (n, n)).astype(np.float32)
    cl = interleaved(n, 4, rng)
    for bad in (4, 0xFFFFFFFF):
        wrong = cl.copy()
        wrong[n - 1] = bad
        for want in (("node", "stat"), ("node",), ("stat",)):
            with pytest.raises(hg.HgError) as e:
                run_matrix(gctx, a, wrong, 4, want=want)
            assert e.value.status == hg.ERR_INVALID and "n_clusters" in str(e.value)
            against_model(gctx, a, cl, 4)
    with pytest.raises(hg.HgError) as e:
        run_matrix(gctx, a, cl, 0)  # (no id is below 0)
    assert e.value.status == hg.ERR_INVALID
    against_model(gctx, a, cl, 4)


def test_no_items(gctx):
    c, hg, dev = gctx
    d_node, d_stat = out_buffers(dev, 0, 3)
    c.cluster_stats_matrix_dev(None, 0, None, 3, None, d_stat.data_ptr())
    assert_same((None, records(d_stat, 3, st.CLUSTER_DTYPE)), st.stats_model(np.zeros((0, 0), np.float32), [], 3))
    c.cluster_stats_dev(None, None, 0, 4096, None, 3, d_node.data_ptr(), None)
    node, stat = c.cluster_stats(np.zeros((0, 4096), np.int16), np.zeros(0, np.int32), np.zeros(0, np.uint32), 2)
    assert node.size == 0
    assert_same((None, stat), st.stats_model(np.zeros((0, 0), np.float32), [], 2))


# ---- real sketches against the oracle ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def real_sketches(gctx):
    c, hg, dev = gctx
    from oracle import oracle as orc
    orc.lib()
    # four roots, members at 0 .. 9.8 % substitutions (synth_genome: member m of a cluster carries m * 0.1 %)
    ids = [r * 100 + m for r in range(4) for m in range(0, 100, 2)]
    seqs = [orc.synth_genome(g, 60_000) for g in ids]
    hv, n2, nh = c.sketch_batch(seqs, hg.default_params(scaled=60))
    mats = {cr.MASH: orc.ani_matrix(hv, n2, hv, n2, 21),
            cr.MAX_CONTAINMENT: cr.ani_ref(orc, cr.exact_dots(hv, hv), n2[:, None], n2[None, :], 21, cr.MAX_CONTAINMENT)}
    return hv, n2, mats


@pytest.mark.parametrize("metric", [cr.MASH, cr.MAX_CONTAINMENT])
def test_real_sketches_against_oracle(gctx, real_sketches, metric):
    c, hg, dev = gctx
    hv, n2, mats = real_sketches
    c.set_ani_metric(metric)
    seen = set()
    for th in (95.0, 99.0):
        for how in ("single", "greedy", "average"):
            if how == "single":
                rep, cl, nc = c.cluster(hv, n2, 21, th)
            elif how == "greedy":
                rep, cl, ani, nc = c.cluster_greedy(hv, n2, 21, th)
            else:
                rep, cl, into, level, size, nc = c.cluster_average(hv, n2, 21, th)
            want = st.stats_model(mats[metric], cl, nc)
            assert_same(c.cluster_stats(hv, n2, cl, nc, 21), want)
            assert (want[1]["size"] > 0).all() and int(want[1]["size"].sum()) == hv.shape[0]
            seen.add(nc)
    assert len(seen) > 1 and max(seen) > 4


def test_directional_metric_is_invalid(gctx, real_sketches):
    c, hg, dev = gctx
    hv, n2, mats = real_sketches
    c.set_ani_metric(cr.CONTAINMENT)
    with pytest.raises(hg.HgError) as e:
        c.cluster_stats(hv, n2, np.zeros(hv.shape[0], np.uint32), 1, 21)
    assert e.value.status == hg.ERR_INVALID
    assert "HG_ANI_CONTAINMENT is directional" in str(e.value)


# ---- hg_cluster_stats_dev on the bench's clustered HVs -----------------------------------------------------------------
N_BENCH = 1_000


@pytest.fixture(scope="module")
def clustered(gctx):
    """(hv, n2, hg_dist_full_dev's matrix on the host, median within-cluster ANI of rows 0..299)"""
    import torch
    c, hg, dev = gctx
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import bench
    hv = bench.clustered_hvs(N_BENCH, 0, dev)
    n2 = (hv.int() ** 2).sum(1).int()
    full = torch.empty(N_BENCH * N_BENCH, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    c.dist_full_dev(hv.data_ptr(), n2.data_ptr(), N_BENCH, hv.data_ptr(), n2.data_ptr(), N_BENCH, hv.shape[1], 21, full.data_ptr())
    c.sync()
    full = full.cpu().numpy().reshape(N_BENCH, N_BENCH)
    i, j = np.triu_indices(300, 1)
    within = full[i, j][i // 100 == j // 100]  # (clustered_hvs: groups of 100 consecutive rows)
    return hv, n2, full, float(np.median(within))


def assign(c, hv, n2, th, how, n=N_BENCH):
    """the device assignment of hg_cluster_dev / hg_cluster_average_dev: (ids on the device, count)"""
    import torch
    rep = torch.zeros(n, dtype=torch.int32, device=hv.device)
    cl = torch.zeros(n, dtype=torch.int32, device=hv.device)
    torch.cuda.synchronize()
    fn = c.cluster_dev if how == "single" else c.cluster_average_dev
    nc = fn(hv.data_ptr(), n2.data_ptr(), n, hv.shape[1], rep.data_ptr(), cl.data_ptr(), ksize=21, ani_th=th)
    return cl, nc


def stats_dev(c, hv, n2, cl, nc, n=N_BENCH):
    import torch
    d_node, d_stat = out_buffers(hv.device, n, nc)
    torch.cuda.synchronize()
    c.cluster_stats_dev(hv.data_ptr(), n2.data_ptr(), n, hv.shape[1], cl.data_ptr(), nc, d_node.data_ptr(), d_stat.data_ptr(), 21)
    torch.cuda.synchronize()
    return records(d_node, n, st.NODE_DTYPE), records(d_stat, nc, st.CLUSTER_DTYPE)


def test_stats_dev_clustered_in_blocks(gctx, clustered):
    import torch
    c, hg, dev = gctx
    hv, n2, full, median = clustered
    cl, nc = assign(c, hv, n2, 95.0, "single")
    h_cl = cl.cpu().numpy().view(np.uint32)
    want = st.stats_model(full, h_cl, nc)
    assert_same(stats_dev(c, hv, n2, cl, nc), want)
    for rows in ("7", "64", "1000"):
        c.set_debug("stats_block_rows", rows)
        assert_same(stats_dev(c, hv, n2, cl, nc), want)
    c.set_debug("stats_block_rows", "0")
    c.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    try:
        assert_same(stats_dev(c, hv, n2, cl, nc), want)
    finally:
        c.reset_stream()
    # the host form, on the first 300 rows (three groups) with an assignment of its own
    h_hv, h_n2 = hv[:300].cpu().numpy(), n2[:300].cpu().numpy()
    own = (np.arange(300) // 100 * 2 + (np.arange(300) % 7 == 0)).astype(np.uint32)
    assert_same(c.cluster_stats(h_hv, h_n2, own, 6, 21), st.stats_model(full[:300, :300], own, 6))
    assert_same(c.cluster_stats(h_hv, h_n2, own, 6, 21, node=False), st.stats_model(full[:300, :300], own, 6))
    assert_same(c.cluster_stats(h_hv, h_n2, own, 6, 21, stat=False), st.stats_model(full[:300, :300], own, 6))


def test_the_statistics_show_the_chaining_of_single_linkage(gctx, clustered):
    c, hg, dev = gctx
    hv, n2, full, median = clustered
    th_milli = av.th_milli(median)
    cl, nc = assign(c, hv, n2, median, "single")
    node, single = stats_dev(c, hv, n2, cl, nc)
    assert_same((node, single), st.stats_model(full, cl.cpu().numpy().view(np.uint32), nc))
    pairs = single["size"] >= 2
    assert pairs.any() and (single["within_min"][pairs] < th_milli).any()  # members joined by a path, not by their own ANI
    cl, nc_avg = assign(c, hv, n2, median, "average")
    node, average = stats_dev(c, hv, n2, cl, nc_avg)
    assert_same((node, average), st.stats_model(full, cl.cpu().numpy().view(np.uint32), nc_avg))
    pairs = average["size"] >= 2
    mean_milli = average["within_sum"][pairs].astype(np.float64) / (average["size"][pairs].astype(np.float64) * (average["size"][pairs] - 1))
    assert pairs.any() and (mean_milli >= average["within_min"][pairs]).all()
    print("median %.3f: single linkage %d clusters (lowest within ANI %.3f), average linkage %d (lowest mean %.3f)"
          % (median, nc, single["within_min"][single["size"] >= 2].min() / 1000.0, nc_avg, mean_milli.min() / 1000.0))
    assert nc_avg > nc


# ---- command line ------------------------------------------------------------------------------------------------------
def write_fasta(path, seq, name):
    s = bytes(seq).decode()
    with open(path, "w") as f:
        f.write(">%s\n" % name)
        for i in range(0, len(s), 80):
            f.write(s[i:i + 80] + "\n")


def cli(hg, *args):
    r = subprocess.run([hg.CLI_PATH] + list(args), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return r


def test_cli_stats_end_to_end(gctx, tmp_path):
    c, hg, dev = gctx
    from oracle import oracle as orc
    orc.lib()
    d = tmp_path / "fa"
    d.mkdir()
    ids = [40, 35, 0, 3, 199, 101, 140, 100, 300]
    for k, g in enumerate(ids):
        write_fasta(str(d / ("f%02d_g%03d.fna" % (k, g))), orc.synth_genome(g, 200_000)[1:], "g%d" % g)
    sk = str(tmp_path / "all.sketch")
    cli(hg, "sketch", "-p", str(d), "-o", sk, "-s", "100", "-t", "4")
    recs = hg.read_sketch_file(sk)
    files = [x["file_str"] for x in recs]
    n = len(files)
    # model: oracle sketches of the same files, the oracle's ANI matrix
    hvs, n2s = [], []
    for f in files:
        hv, n2, _ = orc.sketch_genome(hg.read_merge_seq(f), ksize=21, scaled=100, norm=orc.NORM_U2T)
        hvs.append(hv), n2s.append(n2)
    hvs, n2s = np.stack(hvs), np.array(n2s, np.int32)
    assert n2s.tolist() == [x["hv_norm_2"] for x in recs]
    ani = orc.ani_matrix(hvs, n2s, hvs, n2s, 21)
    counts = set()
    schemes = {"single": ("--linkage", "single"), "greedy": ("--linkage", "greedy", "--order", "size"),
               "setcover": ("--linkage", "setcover"), "average": ("--hclust", "average")}
    for th, hows in (("95", tuple(schemes)), ("97.5", ("single",))):
        for how in hows:
            flags = schemes[how]
            plain, out, stats = (str(tmp_path / ("%s%s_%s.tsv" % (how, th, x))) for x in ("plain", "out", "stats"))
            r = cli(hg, "cluster", "-p", sk, "-o", out, "-a", th, *flags, "--stats", stats)
            if th == "95":  # -o does not know of --stats
                cli(hg, "cluster", "-p", sk, "-o", plain, "-a", th, *flags)
                assert open(out, "rb").read() == open(plain, "rb").read()
            # the statistics describe the clusters -o names, computed in processing order
            by_file = {line.split("\t")[0]: int(line.split("\t")[1]) for line in open(out).read().splitlines()}
            order = np.argsort(-n2s.astype(np.int64), kind="stable") if how == "greedy" else np.arange(n)
            cl = np.array([by_file[files[i]] for i in order], np.uint32)
            nc = int(cl.max()) + 1
            nodes, model = st.stats_model(ani[np.ix_(order, order)], cl, nc)
            want = st.stats_lines(model, cl, [files[i] for i in order])
            assert open(stats, "rb").read() == want.encode()
            assert ("Output statistics of %d clusters (%d not separated) to file %s" % (nc, st.not_separated(model), stats)) in r.stdout
            lines = r.stdout.splitlines()
            at = [k for k, x in enumerate(lines) if "Output statistics of" in x]
            assert len(at) == 1 and "Output %d genomes in %d clusters" % (n, nc) in lines[at[0] - 1]
            counts.add(nc)
    assert len(counts) > 1 and max(counts) > 1 and min(counts) < n
    # with --tree and --levels the statistics are those of -a
    out, stats, tree = (str(tmp_path / x) for x in ("lv_out.tsv", "lv_stats.tsv", "lv_tree.tsv"))
    cli(hg, "cluster", "-p", sk, "-o", out, "-a", "95", "--tree", tree, "--levels", "97.5", "--stats", stats)
    assert open(stats, "rb").read() == open(str(tmp_path / "single95_stats.tsv"), "rb").read()
