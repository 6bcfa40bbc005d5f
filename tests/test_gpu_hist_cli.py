"""`hyper-gen dist --histogram` end to end.  The sketches are the windows of the seeded genomes of tests/test_gpu_frag_cli.py (A; B = A
with 3 % substitutions and its middle replaced; C and D unrelated), 60 records a file: related windows in the nineties, the rest
at 0 or in the noise.  Every run writes its `dist -a 0` TSV and its histogram, and the histogram file equals, byte for byte,
what tests/hist_ref.py makes of the third field of THAT TSV -- on two files (all pairs), on one file (i < j) and on one file under
containment (i != j), at the default width, 1, 0.001 and 100.  -o is what it is without the option, at -a 95 too, and the
option goes with --columns and --newick."""
import subprocess

import pytest

import hist_ref
import test_gpu_frag_cli as fcli

pytestmark = pytest.mark.gpu

WINDOW = 4000
FORMS = {"two_files": ("ref", "qry", ()), "one_file": ("qry", "qry", ()), "one_file_containment": ("qry", "qry", ("--ani_metric", "containment"))}


@pytest.fixture(scope="module")
def hg():
    import hypergen_amd
    hypergen_amd.lib_hist()
    return hypergen_amd


@pytest.fixture(scope="module")
def sketched(hg, tmp_path_factory):
    root = tmp_path_factory.mktemp("histogram")
    g = fcli.genomes()
    for side, members in (("ref", "ad"), ("qry", "bc")):
        d = root / side
        d.mkdir()
        for m in members:
            (d / (m + ".fna")).write_bytes(fcli.fasta("genome_" + m, g[m]))
        log = fcli.cli(hg, "sketch", "-p", str(d), "-o", str(root / (side + ".sketch")), "-s", str(fcli.SCALED), "-t", "2", "--fragment", str(WINDOW))
        assert "Sketching 60 windows of 2 files took" in log
    return root


def dist(hg, root, form, out, *more):
    r, q, metric = FORMS[form]
    return fcli.cli(hg, "dist", "-r", str(root / (r + ".sketch")), "-q", str(root / (q + ".sketch")), "-o", str(out), *metric, *more)


@pytest.mark.parametrize("width", [None, "1", "0.001", "100"])
@pytest.mark.parametrize("form", list(FORMS))
def test_histogram_equals_the_histogram_of_the_runs_own_tsv(hg, sketched, tmp_path, form, width):
    w = hist_ref.parse_bin(width or "0.1")
    log = dist(hg, sketched, form, tmp_path / "d.tsv", "-a", "0", "--histogram", str(tmp_path / "h.tsv"), *(("--histogram_bin", width) if width else ()))
    tsv = (tmp_path / "d.tsv").read_text()
    pairs = {"two_files": 60 * 60, "one_file": 60 * 59 // 2, "one_file_containment": 60 * 59}[form]
    assert tsv.count("\n") == pairs  # -a 0 writes every pair dist enumerates
    m = hist_ref.tsv_milli(tsv)
    assert (m == 0).sum() > pairs // 10 and len(set(m.tolist())) > 50  # (the input: many zeros and many different values)
    want = hist_ref.file_text(hist_ref.counts_of_milli(m, w), w)
    got = (tmp_path / "h.tsv").read_text()
    assert got == want
    assert got.count("\n") == hist_ref.bins(w) and got.splitlines()[0].split("\t")[3] == str(pairs)
    assert "Output ANI histogram of %d pairs in %d bins of width %s to file %s" % (pairs, hist_ref.bins(w), hist_ref.milli_str(w), tmp_path / "h.tsv") in log


@pytest.mark.parametrize("form", list(FORMS))
def test_the_tsv_is_what_it_is_without_the_option(hg, sketched, tmp_path, form):
    for a in ("95", "0"):
        dist(hg, sketched, form, tmp_path / "plain.tsv", "-a", a)
        dist(hg, sketched, form, tmp_path / "with.tsv", "-a", a, "--histogram", str(tmp_path / ("h%s.tsv" % a)), "--histogram_bin", "0.5")
        assert (tmp_path / "plain.tsv").read_bytes() == (tmp_path / "with.tsv").read_bytes()
        if a == "0" or form == "two_files":  # (the windows of one file share nothing: none of its pairs reaches 95)
            assert (tmp_path / "plain.tsv").stat().st_size > 0
    # -a is not applied to the histogram
    assert (tmp_path / "h95.tsv").read_bytes() == (tmp_path / "h0.tsv").read_bytes()


def test_it_goes_with_columns_and_newick(hg, sketched, tmp_path):
    more = ("-a", "0", "--columns", "containment,mash", "--newick", str(tmp_path / "t.nwk"))
    dist(hg, sketched, "one_file", tmp_path / "plain.tsv", *more)
    tree = (tmp_path / "t.nwk").read_bytes()
    dist(hg, sketched, "one_file", tmp_path / "with.tsv", *more, "--histogram=" + str(tmp_path / "h.tsv"))
    assert (tmp_path / "plain.tsv").read_bytes() == (tmp_path / "with.tsv").read_bytes() and (tmp_path / "t.nwk").read_bytes() == tree
    m = hist_ref.tsv_milli((tmp_path / "with.tsv").read_text())
    assert (tmp_path / "h.tsv").read_text() == hist_ref.file_text(hist_ref.counts_of_milli(m, 100), 100)


def test_a_refused_run_writes_nothing(hg, sketched, tmp_path):
    r = subprocess.run([hg.CLI_PATH, "dist", "-r", str(sketched / "ref.sketch"), "-q", str(sketched / "qry.sketch"), "-o", str(tmp_path / "d.tsv"),
                        "--histogram", str(tmp_path / "h.tsv"), "--histogram_bin", "0.0005"], capture_output=True, text=True)
    assert r.returncode == 2 and "invalid value '0.0005' for '--histogram_bin'" in r.stderr and not list(tmp_path.iterdir())
