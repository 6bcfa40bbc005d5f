"""The command line's TSV writer at its seams: `dist`, `search`, `cluster -o` and `cluster --tree` all format their lines on
-t threads, one part per 4096 lines at the most, and write the parts side by side.  The cases sit on both sides of 4096 lines
and beyond two parts; every dist and search case runs with -t 1 and -t 16 and must write the same bytes both times -- the
lines built here from the library's own results (hg_dist + hg_sort_ani_hits, hg_search_topk, hg_ani_pairs), printed with
"%.3f", which for the dist cases are also the oracle's lines (test_gpu_cli.oracle_tsv).  -a 0 makes every pair a line (ANI is
clamped to [0, 100]), so the line counts are exact."""
import subprocess

import numpy as np
import pytest

import ani_pairs_ref as ap
import cluster_greedy_ref as gr
import cluster_tree_ref as tr
import containment_ref as cr
from test_gpu_cli import oracle_tsv

pytestmark = pytest.mark.gpu
K, HV_D = 21, 1024


@pytest.fixture(scope="module")
def env(tmp_path_factory):
    """two sets of 96 sketches in clusters of 8 (ANIs from ~97 down to 0), 40 more with loners among them, a Context"""
    import torch
    import bench
    import hypergen_amd as hg
    dev = torch.device("cuda:0")
    tmp = tmp_path_factory.mktemp("cli_writer")

    def rows(n, first=0, salt=0):
        return bench.clustered_hvs(n, first, dev, n=900, cluster=8, salt=salt).cpu().numpy()[:, :HV_D].copy()

    sets = {"a": rows(96), "b": rows(96, salt=1),
            # 4 clusters of 8 and 8 sketches that are each the only one of their cluster
            "c": np.concatenate([rows(32)] + [rows(1, 1000 + 8 * j) for j in range(8)])}
    files = {}

    def side(tag, m):
        """the first m sketches of a set as a .sketch file: (path, names, hv, n2)"""
        if (tag, m) not in files:
            hv = sets[tag][:m]
            n2 = cr.norms(hv)
            names = ["/d/%s/%s%04d.fna" % (tag, "x" * (i * 5 % 7), i) for i in range(m)]
            recs = []
            for i in range(m):
                q, pk = hg.hv_pack(hv[i])
                recs.append(dict(ksize=K, scaled=1500, canonical=True, seed=123, hv_d=HV_D, hv_quant_bits=q, hv_norm_2=int(n2[i]),
                                 file_str=names[i], hv=pk.view(np.int16)))
            path = str(tmp / ("%s%d.sketch" % (tag, m)))
            hg.write_sketch_file(path, recs)
            files[(tag, m)] = (path, names, hv, n2)
        return files[(tag, m)]

    with hg.Context(0) as ctx:
        yield {"hg": hg, "ctx": ctx, "tmp": tmp, "side": side}


def run_both(env, args, name):
    """the command with -t 1 and with -t 16: the bytes of the one file both must write"""
    outs = []
    for t in ("1", "16"):
        out = str(env["tmp"] / ("%s_t%s.tsv" % (name, t)))
        r = subprocess.run([env["hg"].CLI_PATH] + args + ["-o", out, "-t", t], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        outs.append(open(out, "rb").read())
    assert outs[0] == outs[1], name
    return outs[0].decode()


def dist_lines(env, R, Q, sym, metric=cr.MASH, ani_th=0.0):
    """(hits in dump order, their lines) from the library: hg_dist, hg_sort_ani_hits; one file under the directional metric =
    the full comparison without the pairs i = j"""
    ctx, hg = env["ctx"], env["hg"]
    full = sym and metric == cr.CONTAINMENT
    ctx.set_ani_metric(metric)
    try:
        hits = ctx.dist(R[2], R[3], Q[2], Q[3], K, symmetric=sym and not full, ani_th=ani_th)
    finally:
        ctx.set_ani_metric(cr.MASH)
    if hits.size:
        hits = hg.sort_ani_hits(hits, len(Q[1]), symmetric=sym and not full)
    if full:
        hits = hits[hits["ref_idx"] != hits["qry_idx"]]
    return hits, "".join("%s\t%s\t%.3f\n" % (R[1][h["ref_idx"]], Q[1][h["qry_idx"]], float(h["ani"])) for h in hits)


# (reference sketches, query sketches or None for the one file against itself, lines, formatter parts at -t 16)
DIST = [(63, 65, 4095, 1), (64, 64, 4096, 2), (96, 96, 9216, 3), (91, None, 4095, 1), (92, None, 4186, 2)]


@pytest.mark.parametrize("nr,nq,lines,parts", DIST, ids=["%dx%s" % (c[0], c[1] or "self") for c in DIST])
def test_dist_on_both_sides_of_a_part(env, orc, nr, nq, lines, parts):
    R = env["side"]("a", nr)
    Q = env["side"]("b", nq) if nq else R
    sym = nq is None
    assert lines == (nr * (nr - 1) // 2 if sym else nr * nq) and parts == min(16, lines // 4096 + 1)
    hits, want = dist_lines(env, R, Q, sym)
    assert len(hits) == lines and want == oracle_tsv(orc, R[2], R[3], Q[2], Q[3], R[1], Q[1], K, 0.0, sym)
    assert len({l.rsplit("\t", 1)[1] for l in want.splitlines()}) > 50  # the ANIs vary
    assert run_both(env, ["dist", "-r", R[0], "-q", Q[0], "-a", "0"], "dist_%d_%s" % (nr, nq)) == want


def test_dist_one_file_under_containment_writes_every_ordered_pair(env, orc):
    R = env["side"]("a", 92)
    hits, want = dist_lines(env, R, R, True, cr.CONTAINMENT)
    assert len(hits) == 92 * 91 == 8372
    ani = cr.ani_ref(orc, cr.exact_dots(R[2], R[2]), R[3][:, None], R[3][None, :], K, cr.CONTAINMENT)
    every = oracle_tsv(orc, R[2], R[3], R[2], R[3], R[1], R[1], K, 0.0, False, ani=ani)
    assert want == "".join(l for l in every.splitlines(True) if l.split("\t")[0] != l.split("\t")[1])
    assert run_both(env, ["dist", "-r", R[0], "-q", R[0], "-a", "0", "--ani_metric", "containment"], "dist_cont") == want


COLS = ["containment_ref", "mash"]  # wider lines, and not in the order of the column bits


@pytest.fixture(scope="module")
def wide(env, orc):
    """64 x 64: the plain lines and the lines with COLS, from hg_dist and hg_ani_pairs (whose values are the reference's)"""
    R, Q = env["side"]("a", 64), env["side"]("b", 64)
    hits, plain = dist_lines(env, R, Q, False)
    mask = ap.CONTAINMENT_REF | ap.MASH
    v = env["ctx"].ani_pairs(R[2], R[3], Q[2], Q[3], hits, mask, K)
    dots = cr.exact_dots(R[2], Q[2])[hits["ref_idx"], hits["qry_idx"]]
    assert ap.bits_equal(v, ap.columns(orc, mask, dots, R[3][hits["ref_idx"]], Q[3][hits["qry_idx"]], K))
    assert ap.bits_equal(v[:, ap.place(mask, ap.MASH)], hits["ani"])
    want = "".join("%s\t%s\t%.3f\t%.3f\t%.3f\n" % (R[1][h["ref_idx"]], Q[1][h["qry_idx"]], float(h["ani"]),
                                                  float(x[ap.place(mask, ap.CONTAINMENT_REF)]), float(x[ap.place(mask, ap.MASH)]))
                   for h, x in zip(hits, v))
    assert want.count("\n") == plain.count("\n") == 4096
    fed = str(env["tmp"] / "fed.tsv")
    open(fed, "w").write(plain)
    return ["dist", "-r", R[0], "-q", Q[0], "-a", "0"], fed, plain, want


def test_dist_columns(env, wide):
    base, fed, plain, want = wide
    assert run_both(env, base + ["--columns", ",".join(COLS)], "dist_cols") == want


@pytest.mark.parametrize("with_columns", [False, True], ids=["plain", "columns"])
def test_dist_lines_fed_back_as_pairs(env, wide, with_columns):
    base, fed, plain, want = wide
    extra = ["--columns", ",".join(COLS)] if with_columns else []
    assert run_both(env, base + ["--pairs", fed] + extra, "dist_pairs%d" % with_columns) == (want if with_columns else plain)


def search_lines(env, R, Q, k, ani_th=0.0):
    top, cnt = env["ctx"].search_topk(R[2], R[3], Q[2], Q[3], K, ani_th=ani_th, k=k)
    return "".join("%s\t%s\t%.3f\n" % (Q[1][q], R[1][top[q, r]["ref_idx"]], float(top[q, r]["ani"]))
                   for q in range(len(Q[1])) for r in range(min(int(cnt[q]), k)))


# (-n, --search_path, results): 6144 results are two parts, whose seam lies inside a query's results
SEARCH = [(64, "topk", 6144), (64, "hits", 6144), (1, "auto", 96)]


@pytest.mark.parametrize("k,path,results", SEARCH, ids=["n%d_%s" % c[:2] for c in SEARCH])
def test_search_results_across_parts_and_both_paths(env, k, path, results):
    R, Q = env["side"]("a", 96), env["side"]("b", 96)
    want = search_lines(env, R, Q, k)
    assert want.count("\n") == results == 96 * k
    got = run_both(env, ["search", "-r", R[0], "-q", Q[0], "-a", "0", "-n", str(k), "--search_path", path], "search_%d_%s" % (k, path))
    assert got == want


@pytest.mark.parametrize("mode", ["dist", "search"])
def test_no_hit_writes_an_empty_file(env, mode):
    R, Q = env["side"]("a", 63), env["side"]("b", 65)
    assert (dist_lines(env, R, Q, False, ani_th=100.5)[1] if mode == "dist" else search_lines(env, R, Q, 1, ani_th=100.5)) == ""
    assert run_both(env, [mode, "-r", R[0], "-q", Q[0], "-a", "100.5"], mode + "_empty") == ""


@pytest.fixture(scope="module")
def forty(env, orc):
    """the 40 sketches with loners, the oracle's ANI matrix and three thresholds: a floor between the ANIs across clusters
    (up to ~89: Mash ANI is logarithmic) and those within one (~96-97), and two levels inside the latter's range (written so that
    the command line reads back the same float32)"""
    C = env["side"]("c", 40)
    ani = orc.ani_matrix(C[2], C[3], C[2], C[3], K)
    same = np.zeros((40, 40), bool)
    for g in range(4):
        same[8 * g: 8 * g + 8, 8 * g: 8 * g + 8] = True
    iu = np.triu_indices(40, 1)
    within, across = np.sort(ani[iu][same[iu]]), ani[iu][~same[iu]]
    floor, lo, hi = 93.0, float(within[within.size // 2]), float(within[within.size * 9 // 10])
    assert across.max() < floor < within[0] and lo < hi
    return C, ani, floor, lo, hi


def test_cluster_lines_levels_and_tree(env, forty):
    C, ani, floor, lo, hi = forty
    files, n = C[1], 40
    tree, rep, cl, nc = tr.tree_model_matrix(ani, floor)
    sizes = np.bincount(cl)
    assert nc == 12 and (sizes == 1).sum() == 8 and (sizes == 8).sum() == 4  # singletons and clusters with members
    cuts = [(rep, cl, nc)] + [tr.cut(n, tree, t) for t in (lo, hi)]
    assert nc <= cuts[1][2] <= cuts[2][2] and nc < cuts[2][2] < n  # (a tenth of the ANIs within clusters reach the last level)
    want_tree = "".join("%s\t%s\t%.3f\n" % (files[e["ref_idx"]], files[e["qry_idx"]], float(e["ani"])) for e in tree)
    want_out = "".join("\t".join([files[i]] + [x for r_, c_, _ in cuts for x in (str(c_[i]), files[r_[i]])]) + "\n" for i in range(n))
    tf = str(env["tmp"] / "tree.tsv")
    got = run_both(env, ["cluster", "-p", C[0], "-a", "%.9g" % floor, "--tree", tf, "--levels", "%.9g,%.9g" % (lo, hi)], "cluster_levels")
    assert got == want_out and open(tf).read() == want_tree and want_tree.count("\n") == n - nc


def test_cluster_greedy_by_size(env, forty):
    C, ani, floor, lo, hi = forty
    files, n = C[1], 40
    perm = np.argsort(-C[3].astype(np.int64), kind="stable")
    assert not np.array_equal(perm, np.arange(n))
    rep, cl, v, nc = gr.greedy_model_matrix(ani[np.ix_(perm, perm)], lo)
    pos = np.argsort(perm)
    assert 12 <= nc < n and (np.bincount(cl) > 1).any() and (np.bincount(cl) == 1).sum() >= 8  # (the loners at the least)
    want = "".join("%s\t%d\t%s\t%.3f\n" % (files[i], cl[pos[i]], files[perm[rep[pos[i]]]], float(v[pos[i]])) for i in range(n))
    assert run_both(env, ["cluster", "-p", C[0], "-a", "%.9g" % lo, "--linkage", "greedy", "--order", "size"], "cluster_greedy") == want
