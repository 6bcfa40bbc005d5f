"""`hyper-gen dist --columns` and `dist --pairs` end to end: the lines of the plain run with further fields, and the listed
pairs in the order of the list -- every field EQUAL to the text of the reference value (tests/ani_pairs_ref.py) computed from
the HVs the .sketch files hold."""
import os
import subprocess

import numpy as np
import pytest

import ani_pairs_ref as ap
import containment_ref as cr

pytestmark = pytest.mark.gpu
K = 21
COLS = ["containment", "containment_ref", "max_containment", "mash"]


@pytest.fixture(scope="module")
def hg():
    import hypergen_amd
    return hypergen_amd


def run(hg, *args):
    return subprocess.run([hg.CLI_PATH, *args], capture_output=True, text=True, timeout=300)


@pytest.fixture(scope="module")
def files(hg, tmp_path_factory):
    """12 sketches from one `sketch` run -- three 60 kbp parents, each with a 1 % mutant and a 30 % and a 60 % fragment of the
    mutant -- written again as a.sketch (parents and mutants), b.sketch (fragments) and all.sketch"""
    tmp = tmp_path_factory.mktemp("ani_pairs_cli")
    d = tmp / "fna"
    d.mkdir()
    for i in range(3):
        p = cr.synth(300 + i, 60_000)
        m = cr.mutate(p, 0.01, 40 + i)
        for name, seq in (("p%d_parent" % i, p), ("p%d_mutant" % i, m), ("p%d_frag30" % i, cr.fragment(m, 0.3, i)),
                          ("p%d_frag60" % i, cr.fragment(m, 0.6, 7 + i))):
            cr.write_fasta(str(d / (name + ".fna")), seq, name)
    sk = str(tmp / "all.sketch")
    r = run(hg, "sketch", "-p", str(d), "-o", sk, "-s", "200", "-t", "4")
    assert r.returncode == 0, r.stderr
    recs = hg.read_sketch_file(sk)
    assert len(recs) == 12
    a = [x for x in recs if "frag" not in x["file_str"]]
    b = [x for x in recs if "frag" in x["file_str"]]
    hg.write_sketch_file(str(tmp / "a.sketch"), a)
    hg.write_sketch_file(str(tmp / "b.sketch"), b)

    def side(rs):
        hv = np.stack([hg.hv_unpack(x["hv"].view(np.uint8), x["hv_d"], x["hv_quant_bits"]) for x in rs])
        return {"names": [x["file_str"] for x in rs], "hv": hv, "n2": cr.wrap_i32([x["hv_norm_2"] for x in rs]), "path": None}

    out = {"tmp": tmp, "a": side(a), "b": side(b), "all": side(recs)}
    for k in ("a", "b", "all"):
        out[k]["path"] = str(tmp / (k + ".sketch"))
        out[k]["index"] = {}
        for i, n in enumerate(out[k]["names"]):
            out[k]["index"].setdefault(n, i)
    return out


def want_fields(orc, R, Q, i, j, names):
    """the text of the listed columns for pair (i, j)"""
    dot = cr.exact_dots(R["hv"][i: i + 1], Q["hv"][j: j + 1])[0, 0]
    v = ap.columns(orc, ap.ALL, [dot], [R["n2"][i]], [Q["n2"][j]], K)[0]
    return [ap.fmt3(v[ap.place(ap.ALL, ap.NAMES[n])]) for n in names]


def check_columns(hg, orc, files, r_key, q_key, extra, cols):
    """dist with and without --columns: the same lines, and the further fields are the reference's"""
    R, Q = files[r_key], files[q_key]
    plain, wide = str(files["tmp"] / "plain.tsv"), str(files["tmp"] / "wide.tsv")
    base = ["dist", "-r", R["path"], "-q", Q["path"], "-a", "80", *extra]
    r = run(hg, *base, "-o", plain)
    assert r.returncode == 0, r.stderr
    r = run(hg, *base, "-o", wide, "--columns", ",".join(cols))
    assert r.returncode == 0, r.stderr
    lines = open(wide).read().splitlines()
    assert "".join("\t".join(l.split("\t")[:3]) + "\n" for l in lines) == open(plain).read()
    rows = []
    for l in lines:
        f = l.split("\t")
        assert len(f) == 3 + len(cols)
        i, j = R["index"][f[0]], Q["index"][f[1]]
        assert f[3:] == want_fields(orc, R, Q, i, j, cols), l
        rows.append((f[0], f[1], [float(x) for x in f[2:]]))
    return rows


def test_columns_on_two_files(hg, orc, files):
    rows = check_columns(hg, orc, files, "a", "b", [], COLS)
    assert len(rows) >= 12  # every fragment with its parent and the parent's mutant
    seen = 0
    for rf, qf, v in rows:
        if "frag30" in qf and os.path.basename(rf)[:2] == os.path.basename(qf)[:2]:
            cont, cont_ref, _, mash = v[1:]
            # the query is 30 % of the reference: containment_ref's x is ~0.3 of containment's, 100 * ln(1 / 0.3) / 21 = 5.7
            # below it; 3.8 (a ratio of 0.45) leaves room for the sampling noise of ~90 hashes
            assert cont >= mash and cont - cont_ref >= 3.8, (rf, qf, v)
            seen += 1
    assert seen == 6


@pytest.mark.parametrize("metric", ["mash", "containment"])
def test_columns_on_one_file(hg, orc, files, metric):
    rows = check_columns(hg, orc, files, "all", "all", ["--ani_metric", metric], COLS)
    # (per family: parent, mutant and both fragments against parent and mutant -- 5 unordered pairs, 10 ordered ones)
    assert len(rows) >= (15 if metric == "mash" else 30) and all(rf != qf for rf, qf, _ in rows)
    if metric == "containment":  # every ordered pair: both directions of a pair are lines
        assert {(q, r) for r, q, _ in rows if "frag" not in r and "frag" not in q} <= {(r, q) for r, q, _ in rows}
    rows = check_columns(hg, orc, files, "all", "all", ["--ani_metric", metric], [metric])
    assert rows and all(v[0] == v[1] for _, _, v in rows)  # the run's own metric as a column: field 4 is field 3


@pytest.fixture(scope="module")
def pair_list(files):
    A = files["all"]
    rng = np.random.default_rng(21)
    ij = [tuple(int(x) for x in rng.integers(0, 12, 2)) for _ in range(27)]
    ij += [ij[3], (5, 5), (0, 1)]  # a repeated pair, a self pair
    assert len(ij) == 30 and any(i == j for i, j in ij)
    text = "".join("%s\t%s%s\n" % (A["names"][i], A["names"][j], "\tanything 1.5" if n % 4 == 1 else "") for n, (i, j) in enumerate(ij))
    path = str(files["tmp"] / "list.tsv")
    open(path, "w").write(text + "\n")  # (an empty line at the end is not a pair)
    return path, ij


def test_pairs(hg, orc, files, pair_list):
    A, out = files["all"], str(files["tmp"] / "pairs.tsv")
    path, ij = pair_list
    r = run(hg, "dist", "-r", A["path"], "-q", A["path"], "-o", out, "--pairs", path, "-a", "99.9")
    assert r.returncode == 0, r.stderr
    assert ("Output 30 listed ANIs to file " + out) in r.stdout
    want = ["%s\t%s\t%s" % (A["names"][i], A["names"][j], want_fields(orc, A, A, i, j, ["mash"])[0]) for i, j in ij]
    assert open(out).read().splitlines() == want  # list order, -a not applied
    assert sum(l.endswith("\t0.000") for l in want) >= 5 and sum(l.endswith("\t100.000") for l in want) >= 1
    r = run(hg, "dist", "-r", A["path"], "-q", A["path"], "-o", out, "--pairs", path, "--ani_metric", "containment", "--columns",
            "containment_ref,mash")
    assert r.returncode == 0, r.stderr
    want = ["%s\t%s\t%s" % (A["names"][i], A["names"][j], "\t".join(want_fields(orc, A, A, i, j, ["containment", "containment_ref", "mash"])))
            for i, j in ij]
    assert open(out).read().splitlines() == want


def test_pairs_errors_and_empty_list(hg, files, pair_list):
    A, out = files["all"], str(files["tmp"] / "pairs2.tsv")
    path, _ = pair_list
    bad = str(files["tmp"] / "bad.tsv")
    lines = open(path).read().splitlines()[:6]
    lines[4] = "%s\tno_such_genome.fna" % A["names"][0]
    open(bad, "w").write("\n".join(lines) + "\n")
    r = run(hg, "dist", "-r", A["path"], "-q", A["path"], "-o", out, "--pairs", bad)
    assert r.returncode != 0 and "line 5" in r.stderr and "no_such_genome.fna" in r.stderr, r.stderr
    empty = str(files["tmp"] / "empty.tsv")
    open(empty, "w").write("")
    r = run(hg, "dist", "-r", A["path"], "-q", A["path"], "-o", out, "--pairs", empty)
    assert r.returncode == 0 and open(out).read() == "" and "Output 0 listed ANIs" in r.stdout, r.stderr


def test_a_dist_tsv_fed_back_reproduces_itself(hg, files):
    a, b = files["a"], files["b"]
    first, again = str(files["tmp"] / "first.tsv"), str(files["tmp"] / "again.tsv")
    r = run(hg, "dist", "-r", a["path"], "-q", b["path"], "-o", first, "-a", "80")
    assert r.returncode == 0, r.stderr
    r = run(hg, "dist", "-r", a["path"], "-q", b["path"], "-o", again, "--pairs", first)
    assert r.returncode == 0, r.stderr
    assert open(first).read().count("\n") >= 12 and open(again, "rb").read() == open(first, "rb").read()


@pytest.mark.parametrize("flag", [("--columns", "mash"), ("--pairs", "list.tsv")])
def test_shards_are_refused(hg, files, flag):
    a, b = files["a"], files["b"]
    r = run(hg, "dist", "-r", a["path"], "-q", b["path"], "-o", str(files["tmp"] / "s.tsv"), "--shards", "2", *flag)
    assert r.returncode != 0 and "--shards" in r.stderr
