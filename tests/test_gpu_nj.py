"""Neighbour joining on the device (hg_nj*, `hyper-gen dist --newick`): the join array EQUAL, byte for byte, to the models
of tests/nj_ref.py -- the matrix form at sizes on both sides of the 16-byte piece, of the wave and of the scan's start
alignment for rows near the right edge, on clustered matrices, matrices of three values (ties decide nearly every join),
matrices over 0 .. 100 000 (the clamp acts, branches come out negative), matrices with NaN, negative and above-100 entries,
and with garbage below the diagonal; additive matrices just past one and two steps of the row scan, every path length
rebuilt from the joins; resident sketches against the matrix form fed from hg_dist_full_dev, in blocks of several heights,
under both symmetric metrics and through the host form; repeated calls, status codes, and the command line end to end."""
import os
import subprocess
import sys

import numpy as np
import pytest

import containment_ref as cr
import nj_ref as nj

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
    c.set_debug("nj_block_rows", "0")
    c.set_ani_metric(cr.MASH)


def joins_buffer(n, dev):
    import torch
    return torch.full((max(n - 1, 1) * 24,), 0xA5, dtype=torch.uint8, device=dev)


def records(buf, count):
    return buf.cpu().numpy()[:count * 24].view(nj.JOIN_DTYPE)


def run_matrix(gctx, a):
    """hg_nj_matrix_dev on the float matrix a -> the join records"""
    import torch
    c, hg, dev = gctx
    n = a.shape[0]
    d = torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev) if n else None
    out = joins_buffer(n, dev)
    torch.cuda.synchronize()  # (the ctx runs on its own stream)
    count = c.nj_matrix_dev(d.data_ptr() if n else None, n, out.data_ptr())
    assert count == max(n, 1) - 1
    return records(out, count)


def assert_same(got, want):
    want = nj.as_records(want)
    assert got.dtype == want.dtype and got.shape == want.shape
    if got.tobytes() != want.tobytes():
        t = int(np.flatnonzero(got != want)[0])
        raise AssertionError("join %d of %d: got %s, the model has %s" % (t, len(want), got[t], want[t]))


def sym(a):
    a = np.triu(np.asarray(a, np.float32), 1)
    return a + a.T


def matrices(rng, n):
    """the kinds of matrix every size is run on"""
    a = rng.uniform(80.0, 90.0, (n, n))
    g = rng.integers(0, max(2, n // 6), n)  # groups, members scattered over the whole row
    within = g[:, None] == g[None, :]
    a[within] = rng.uniform(96.0, 99.9, int(within.sum()))
    yield "clustered", sym(a)
    yield "three values", sym(rng.choice(np.array([95.0, 97.0, 99.0], np.float32), (n, n)))
    yield "0 .. 100 000", sym(rng.integers(0, 100_001, (n, n)) / 1000.0)
    b = sym(a)
    odd = rng.random((n, n)) < 0.2
    b[odd] = rng.choice(np.array([np.nan, -7.0, 250.0, np.inf, -np.inf, 100.0, 0.0], np.float32), int(odd.sum()))
    yield "NaN, negative and above 100", np.triu(b, 1) + np.triu(b, 1).T
    c = sym(a)
    low = np.tril_indices(n)
    c[low] = rng.choice(np.array([np.nan, 1e30, -1e30, 50.0, 99.0], np.float32), low[0].size)
    yield "garbage below the diagonal", c


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65, 255, 256, 257, 515])
def test_matrix_form_equals_the_model(gctx, n):
    rng = np.random.default_rng(1000 + n)
    negative = 0
    for kind, a in matrices(rng, n):
        d = nj.dist_matrix(a)
        want = nj.nj_model_np(d)
        if n <= 9:
            assert want == nj.nj_model(d), kind
        got = run_matrix(gctx, a)
        try:
            assert_same(got, want)
        except AssertionError as e:
            raise AssertionError("%s, n = %d: %s" % (kind, n, e))
        negative += sum(la < 0 or lb < 0 for _, _, la, lb in want)
    print("n %d: %d joins with a negative branch over the five kinds" % (n, negative))


def test_five_taxa_and_their_ties(gctx):
    c, hg, dev = gctx
    t = np.array([[0, 5, 9, 9, 8], [5, 0, 10, 10, 9], [9, 10, 0, 8, 7], [9, 10, 8, 0, 3], [8, 9, 7, 3, 0]], np.int64) * 1000
    got = run_matrix(gctx, nj.ani_of_milli(t))
    k = 1000 << 15
    assert nj.as_tuples(got) == [(0, 1, 2 * k, 3 * k), (0, 2, 3 * k, 4 * k), (0, 3, 2 * k, 2 * k), (0, 4, 1 * k, 0)]
    assert hg.nj_newick(got, list("abcde")) == ("((('a':0.02000000,'b':0.03000000):0.03000000,'c':0.04000000):0.02000000,"
                                                "'d':0.02000000,'e':0.01000000);")
    # all pairs equal: every join is decided by the names
    got = run_matrix(gctx, sym(np.full((6, 6), 97.0)))
    assert_same(got, nj.nj_model(nj.dist_matrix(sym(np.full((6, 6), 97.0)))))
    assert [(int(x["a"]), int(x["b"])) for x in got] == [(0, 1), (0, 2), (0, 3), (0, 4), (0, 5)]


@pytest.fixture(scope="module")
def additive():
    rng = np.random.default_rng(77)
    return {n: nj.additive_matrix(rng, n) for n in (1025, 2049)}


@pytest.mark.parametrize("n", [1025, 2049])
def test_additive_matrices_are_recovered_exactly(gctx, additive, n):
    """just past one and two 1 024-column steps of the row scan: topology and every branch, from the device's joins alone"""
    t = additive[n]
    got = run_matrix(gctx, nj.ani_of_milli(t))
    joins = nj.as_tuples(got)
    assert np.array_equal(nj.path_lengths(joins, n), t << nj.FRAC_BITS)
    assert all(la >= 0 and lb >= 0 for _, _, la, lb in joins)
    if n == 1025:
        assert_same(got, nj.nj_model_np(t << nj.FRAC_BITS))


# ---- resident sketches ------------------------------------------------------------------------------------------------
N_HV = 300


@pytest.fixture(scope="module")
def clustered(gctx):
    c, hg, dev = gctx
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import bench
    hv = bench.clustered_hvs(N_HV, 0, dev, cluster=25)
    n2 = (hv.int() ** 2).sum(1).int()
    return hv, n2


def nj_dev(gctx, hv, n2, n=N_HV):
    import torch
    c, hg, dev = gctx
    out = joins_buffer(n, dev)
    torch.cuda.synchronize()
    count = c.nj_dev(hv.data_ptr(), n2.data_ptr(), n, hv.shape[1], out.data_ptr(), 21)
    assert count == n - 1
    return records(out, count)


@pytest.mark.parametrize("metric", [cr.MASH, cr.MAX_CONTAINMENT])
def test_resident_sketches_equal_the_matrix_form(gctx, clustered, metric):
    import torch
    c, hg, dev = gctx
    hv, n2 = clustered
    c.set_ani_metric(metric)
    full = torch.empty(N_HV * N_HV, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    c.dist_full_dev(hv.data_ptr(), n2.data_ptr(), N_HV, hv.data_ptr(), n2.data_ptr(), N_HV, hv.shape[1], 21, full.data_ptr())
    c.sync()
    a = full.cpu().numpy().reshape(N_HV, N_HV)
    want = run_matrix(gctx, a)
    assert_same(want, nj.nj_model_np(nj.dist_matrix(a)))
    got = nj_dev(gctx, hv, n2)
    assert got.tobytes() == want.tobytes()
    for rows in ("1", "7", str(N_HV)):
        c.set_debug("nj_block_rows", rows)
        assert nj_dev(gctx, hv, n2).tobytes() == want.tobytes(), rows
    c.set_debug("nj_block_rows", "0")
    # the host form
    host = c.nj(hv.cpu().numpy(), n2.cpu().numpy(), 21)
    assert host.dtype == nj.JOIN_DTYPE and host.tobytes() == want.tobytes()
    print("metric %d: %d of %d joins have a negative branch" % (metric, int(((want["len_a"] < 0) | (want["len_b"] < 0)).sum()), len(want)))


def test_two_calls_give_identical_bytes_and_clustering_still_works(gctx, clustered):
    import torch
    c, hg, dev = gctx
    hv, n2 = clustered

    def complete():
        a = np.full((4, 4), 50.0, np.float32)
        a[0, 1] = a[1, 0] = 99.0
        a[2, 3] = a[3, 2] = 98.0
        d = torch.from_numpy(a).to(dev)
        rep, cl = (torch.zeros(4, dtype=torch.int32, device=dev) for _ in range(2))
        torch.cuda.synchronize()
        count = c.cluster_complete_matrix_dev(d.data_ptr(), 4, 95.0, rep.data_ptr(), cl.data_ptr())
        return count, rep.cpu().numpy().tolist()

    assert complete() == (2, [0, 0, 2, 2])
    first = nj_dev(gctx, hv, n2)
    assert complete() == (2, [0, 0, 2, 2])
    second = nj_dev(gctx, hv, n2)
    assert first.tobytes() == second.tobytes()
    rng = np.random.default_rng(4)
    a = sym(rng.uniform(70.0, 100.0, (130, 130)))
    assert run_matrix(gctx, a).tobytes() == run_matrix(gctx, a).tobytes()
    assert complete() == (2, [0, 0, 2, 2])


def test_status_codes(gctx, clustered):
    import torch
    c, hg, dev = gctx
    hv, n2 = clustered
    d = torch.zeros(16, dtype=torch.float32, device=dev)
    out = joins_buffer(4, dev)
    torch.cuda.synchronize()
    # beyond the limit: refused before anything is allocated (d is never read)
    free_before = torch.cuda.mem_get_info(dev)[0]
    for call in (lambda: c.nj_matrix_dev(d.data_ptr(), hg.NJ_MAX_N + 1, out.data_ptr()),
                 lambda: c.nj_dev(hv.data_ptr(), n2.data_ptr(), hg.NJ_MAX_N + 1, hv.shape[1], out.data_ptr()),
                 lambda: c.nj_dev(hv.data_ptr(), n2.data_ptr(), 1 << 40, hv.shape[1], out.data_ptr())):
        with pytest.raises(hg.HgError) as e:
            call()
        assert e.value.status == hg.ERR_UNSUPPORTED and "HG_NJ_MAX_N" in str(e.value)
    assert torch.cuda.mem_get_info(dev)[0] == free_before
    # NULL arguments
    for call in (lambda: c.nj_matrix_dev(None, 4, out.data_ptr()), lambda: c.nj_matrix_dev(d.data_ptr(), 4, None),
                 lambda: c.nj_dev(None, n2.data_ptr(), 4, hv.shape[1], out.data_ptr()),
                 lambda: c.nj_dev(hv.data_ptr(), None, 4, hv.shape[1], out.data_ptr()),
                 lambda: c.nj_dev(hv.data_ptr(), n2.data_ptr(), 4, hv.shape[1], None)):
        with pytest.raises(hg.HgError) as e:
            call()
        assert e.value.status == hg.ERR_INVALID
    lib = hg.lib()
    assert lib.hg_nj_matrix_dev(c._h, d.data_ptr(), 4, out.data_ptr(), None) == hg.ERR_INVALID  # n_joins == NULL
    assert lib.hg_nj_matrix_dev(None, d.data_ptr(), 4, out.data_ptr(), None) == hg.ERR_INVALID
    # the directional metric: the error clustering gives; the matrix form does not depend on the metric
    c.set_ani_metric(cr.CONTAINMENT)
    with pytest.raises(hg.HgError) as e:
        c.nj_dev(hv.data_ptr(), n2.data_ptr(), 4, hv.shape[1], out.data_ptr())
    assert e.value.status == hg.ERR_INVALID and "HG_ANI_CONTAINMENT is directional" in str(e.value)
    with pytest.raises(hg.HgError) as e:
        c.nj(hv[:4].cpu().numpy(), n2[:4].cpu().numpy())
    assert e.value.status == hg.ERR_INVALID
    a = sym(np.random.default_rng(8).uniform(80.0, 100.0, (9, 9)))
    assert_same(run_matrix(gctx, a), nj.nj_model(nj.dist_matrix(a)))
    c.set_ani_metric(cr.MASH)
    # nothing to join
    assert c.nj_matrix_dev(None, 0, None) == 0 and c.nj_matrix_dev(d.data_ptr(), 1, None) == 0
    assert c.nj_dev(None, None, 0, hv.shape[1], None) == 0 and c.nj_dev(hv.data_ptr(), n2.data_ptr(), 1, hv.shape[1], out.data_ptr()) == 0
    assert len(c.nj(np.zeros((0, 4096), np.int16), np.zeros(0, np.int32))) == 0
    assert len(c.nj(hv[:1].cpu().numpy(), n2[:1].cpu().numpy())) == 0
    two = c.nj(hv[:2].cpu().numpy(), n2[:2].cpu().numpy())
    assert len(two) == 1 and (int(two[0]["a"]), int(two[0]["b"]), int(two[0]["len_b"])) == (0, 1, 0)


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


def test_cli_newick_end_to_end(gctx, tmp_path):
    c, hg, dev = gctx
    from oracle import oracle as orc
    orc.lib()
    d = tmp_path / "fa"
    d.mkdir()
    # four roots, ten members each at 0 .. 9 % substitutions; one name that needs its quote doubled
    ids = [r * 100 + m for r in range(4) for m in range(0, 100, 10)]
    for k, g in enumerate(ids):
        write_fasta(str(d / ("f%02d_g%03d%s.fna" % (k, g, "'s" if k == 3 else ""))), orc.synth_genome(g, 60_000)[1:], "g%d" % g)
    sk = str(tmp_path / "all.sketch")
    cli(hg, "sketch", "-p", str(d), "-o", sk, "-s", "60", "-t", "4")
    files = [x["file_str"] for x in hg.read_sketch_file(sk)]
    n = len(files)
    assert n == 40
    for metric in ("mash", "max_containment"):
        plain, out, tree = (str(tmp_path / ("%s_%s" % (metric, k))) for k in ("plain.tsv", "with.tsv", "tree.nwk"))
        cli(hg, "dist", "-r", sk, "-q", sk, "-o", plain, "-a", "0", "--ani_metric", metric)
        r = cli(hg, "dist", "-r", sk, "-q", sk, "-o", out, "-a", "0", "--ani_metric", metric, "--newick", tree)
        assert open(out, "rb").read() == open(plain, "rb").read()  # -o is what it is without the flag
        assert ("Output neighbour-joining tree of %d genomes to file %s" % (n, tree)) in r.stdout
        # the matrix from the same run's `dist -a 0` values, as text: thousandths
        index = {f: i for i, f in enumerate(files)}
        m = np.zeros((n, n), np.int64)
        lines = [x.split("\t") for x in open(out).read().splitlines()]
        assert len(lines) == n * (n - 1) // 2
        for rf, qf, v in lines:
            whole, frac = v.split(".")
            assert len(frac) == 3
            i, j = sorted((index[rf], index[qf]))
            m[i, j] = m[j, i] = int(whole) * 1000 + int(frac)
        dist = (100_000 - m) << nj.FRAC_BITS
        np.fill_diagonal(dist, 0)
        joins = nj.nj_model_np(dist)
        want = hg.nj_newick(nj.as_records(joins), files)
        assert want == nj.newick_model(joins, files)
        got = open(tree, "rb").read().decode()
        assert got == want and got.count("''") == 1
        assert got.count("(") == n - 2 and got.endswith(");")
    # options that change -o but not the tree's input: the tree does not depend on -a or --columns
    out2, tree2 = str(tmp_path / "th.tsv"), str(tmp_path / "th.nwk")
    cli(hg, "dist", "-r", sk, "-q", sk, "-o", out2, "-a", "95", "--columns", "containment", "--ani_metric", "max_containment", "--newick", tree2)
    assert open(tree2, "rb").read() == open(str(tmp_path / "max_containment_tree.nwk"), "rb").read()
