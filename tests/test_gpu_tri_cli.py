"""`hyper-gen triangle` end to end.  The sketches are windows of the seeded genomes of tests/test_gpu_frag_cli.py (A; B = A with 3 %
substitutions and its middle replaced), 40 records in one file whose directory has a blank in its name: related windows in the
nineties, the rest at 0 or in the noise.  The matrix file equals, byte for byte, what tests/tri_ref.py makes of the same run's
`dist -a 0` TSV -- the lower triangle under mash and max_containment, the square with a diagonal of 100.000 under containment --
whatever -t is; a file of one sketch works; the byte the offset formula names holds the field it should; and dist's own output
is what it is."""
import pytest

import tri_ref
import test_gpu_frag_cli as fcli

pytestmark = pytest.mark.gpu

WINDOW, N = 6000, 40
METRICS = {"mash": tri_ref.LOWER, "max_containment": tri_ref.LOWER, "containment": tri_ref.FULL}


@pytest.fixture(scope="module")
def hg():
    import hypergen_amd
    hypergen_amd.lib_tri()
    return hypergen_amd


@pytest.fixture(scope="module")
def sketched(hg, tmp_path_factory):
    root = tmp_path_factory.mktemp("triangle")
    g = fcli.genomes()
    d = root / "two genomes"
    d.mkdir()
    for m in "ab":
        (d / (m + ".fna")).write_bytes(fcli.fasta("genome_" + m, g[m]))
    log = fcli.cli(hg, "sketch", "-p", str(d), "-o", str(root / "all.sketch"), "-s", str(fcli.SCALED), "-t", "2", "--fragment", str(WINDOW))
    assert "Sketching %d windows of 2 files took" % N in log
    one = root / "one"
    one.mkdir()
    (one / "c.fna").write_bytes(fcli.fasta("genome_c", g["c"][:20_000]))
    fcli.cli(hg, "sketch", "-p", str(one), "-o", str(root / "one.sketch"), "-s", str(fcli.SCALED), "-t", "2")
    return root


@pytest.fixture(scope="module")
def runs(hg, sketched, tmp_path_factory):
    """per metric: the names in file order, the TSV of `dist -a 0`, the matrix file and the log of `triangle`"""
    out = tmp_path_factory.mktemp("runs")
    sk = str(sketched / "all.sketch")
    r = {}
    for metric in METRICS:
        fcli.cli(hg, "dist", "-r", sk, "-q", sk, "-o", str(out / (metric + ".tsv")), "-a", "0", "--ani_metric", metric)
        log = fcli.cli(hg, "triangle", "-p", sk, "-o", str(out / (metric + ".phy")), "--ani_metric", metric)
        tsv, phy = (out / (metric + ".tsv")).read_bytes(), (out / (metric + ".phy")).read_bytes()
        names = [line.split(b"\t")[0] for line in phy.split(b"\n")[1:-1]]
        r[metric] = (names, tsv, phy, log, out / (metric + ".phy"))
    return r


@pytest.mark.parametrize("metric", list(METRICS))
def test_the_matrix_is_the_matrix_of_the_runs_own_tsv(hg, runs, metric):
    names, tsv, phy, log, path = runs[metric]
    layout = METRICS[metric]
    assert len(names) == N == len(set(names)) and all(b" " in n and b":" in n for n in names)  # the names carry the directory's blank
    pairs = N * (N - 1) // 2 if layout == tri_ref.LOWER else N * (N - 1)
    assert tsv.count(b"\n") == pairs  # -a 0 writes every pair dist enumerates
    # the rows stand in the order of the file's records: the windows of a.fna, then those of b.fna, ascending
    assert [n.rsplit(b":", 1)[1] for n in names] == [b"%d-%d" % (s + 1, s + WINDOW) for s in range(0, fcli.LEN, WINDOW)] * 2
    assert all(n.rsplit(b":", 1)[0].endswith(b"two genomes/a.fna" if k < N // 2 else b"two genomes/b.fna") for k, n in enumerate(names))
    want = tri_ref.file_from_tsv(names, tsv, layout)
    assert phy == want
    assert len(phy) == len(b"%d\n" % N) + sum(len(n) + 1 for n in names) + tri_ref.text_bytes(layout, 0, N, N)
    values = {line.rsplit(b"\t", 1)[1] for line in tsv.split(b"\n") if line}
    assert b"0.000" in values and len(values) > 50 and any(v.startswith(b"9") and len(v) == 6 for v in values)  # zeros, noise, the nineties
    what = "lower triangle" if layout == tri_ref.LOWER else "square"
    assert "Output ANI matrix of %d sketches (%s) to file %s" % (N, what, path) in log
    if layout == tri_ref.FULL:
        rows = phy.split(b"\n")[1:-1]
        assert all(row.split(b"\t")[1 + i] == b"100.000" for i, row in enumerate(rows))


@pytest.mark.parametrize("metric", ["mash", "containment"])
def test_the_threads_do_not_show_and_a_is_ignored(hg, sketched, runs, tmp_path, metric):
    sk = str(sketched / "all.sketch")
    for k, more in enumerate((("-t", "1"), ("-t", "8"), ("-t", "3", "-a", "99"))):
        fcli.cli(hg, "triangle", "-p", sk, "-o", str(tmp_path / ("%d.phy" % k)), "--ani_metric", metric, *more)
        assert (tmp_path / ("%d.phy" % k)).read_bytes() == runs[metric][2], more


def test_a_file_of_one_sketch(hg, sketched, tmp_path):
    sk = str(sketched / "one.sketch")
    log = fcli.cli(hg, "triangle", "-p", sk, "-o", str(tmp_path / "l.phy"))
    name = str(sketched / "one" / "c.fna").encode()
    assert (tmp_path / "l.phy").read_bytes() == b"1\n" + name + b"\n" == tri_ref.file_text([name], [[100_000]], tri_ref.LOWER)
    assert "Output ANI matrix of 1 sketches (lower triangle)" in log
    fcli.cli(hg, "triangle", "-p", sk, "-o", str(tmp_path / "f.phy"), "--ani_metric", "containment")
    assert (tmp_path / "f.phy").read_bytes() == b"1\n" + name + b"\t100.000\n"


@pytest.mark.parametrize("metric", list(METRICS))
def test_a_reader_can_seek_to_a_pair(hg, runs, metric):
    names, tsv, phy, log, path = runs[metric]
    layout = METRICS[metric]
    by_pair = {}
    for line in tsv.split(b"\n"):
        if line:
            a, b, v = line.rsplit(b"\t", 2)
            by_pair[a, b] = v
    head = len(b"%d\n" % N)
    for i, j in ((1, 0), (2, 1), (17, 5), (N - 1, 0), (N - 1, N - 2)) + (((0, N - 1), (5, 17)) if layout == tri_ref.FULL else ()):
        at = head + sum(len(n) + 1 for n in names[: i + 1]) + hg.tri_field_offset(layout, 0, i, j, N)
        v = by_pair[names[i], names[j]] if (names[i], names[j]) in by_pair else by_pair[names[j], names[i]]
        last = j == (i - 1 if layout == tri_ref.LOWER else N - 1)
        assert phy[at: at + 8] == v.rjust(7) + (b"\n" if last else b"\t"), (i, j)


def test_dist_is_what_it_is(hg, sketched, runs, tmp_path):
    """the TSV of a threshold run is the `-a 0` TSV's lines at or above it, in their order: the subcommand changed nothing of dist's"""
    sk = str(sketched / "all.sketch")
    fcli.cli(hg, "dist", "-r", sk, "-q", sk, "-o", str(tmp_path / "d.tsv"), "-a", "90")
    got = (tmp_path / "d.tsv").read_bytes()
    lines = [l for l in runs["mash"][1].split(b"\n") if l]
    assert got.count(b"\n") > 5
    for line in got.split(b"\n"):
        assert not line or line in lines
