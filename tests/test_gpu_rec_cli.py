"""`hyper-gen sketch --individual` end to end on the GPU: a directory with two multi-FASTA files, one of them gzip, against plain
`sketch` on a second directory that holds the same records as one file each.  The two .sketch files are equal record for
record, payload bytes included, except for file_str, which is the record's identifier in the first; --min_length drops exactly
the short records; dist prints the identifiers; what the mode refuses once it has read a file."""
import gzip
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BASES = np.frombuffer(b"ACGT", np.uint8)
FIELDS = ("ksize", "canonical", "scaled", "seed", "hv_d", "hv_quant_bits", "hv_norm_2")


@pytest.fixture(scope="module")
def hg():
    import hypergen_amd
    hypergen_amd.lib_rec()
    return hypergen_amd


def fasta(name, seq, width=70, eol=b"\n"):
    return eol.join([b">" + name] + [seq[j:j + width] for j in range(0, len(seq), width)]) + eol


@pytest.fixture(scope="module")
def dirs(tmp_path_factory):
    """(multi-FASTA directory, one-file-per-record directory, the records as (identifier, sequence) in the order sketch reads them)"""
    rng = np.random.default_rng(31)
    root = tmp_path_factory.mktemp("individual")
    multi, single = root / "multi", root / "single"
    multi.mkdir(), single.mkdir()
    lens = {"a": (4000, 30, 2500, 999), "b": (1000, 6000, 12)}
    records = []
    for f in ("a", "b"):
        text = b""
        for i, n in enumerate(lens[f]):
            seq = rng.choice(BASES, n).tobytes()
            if i == 2:
                seq = seq[:1000] + seq[:1000].lower() + seq[2000:]  # lower case and a repeat
            ident = b"%s_contig%d" % (f.encode(), i)
            text += fasta(ident + b" len=%d\tmore words" % n, seq, eol=b"\r\n" if i == 1 else b"\n")
            records.append((ident, seq))
        (multi / ("%s.fna" % f)).write_bytes(text if f == "a" else gzip.compress(text))
    # one file per record, named so that sketch reads them in the same order (glob order of *.fna)
    for j, (ident, seq) in enumerate(records):
        (single / ("r%02d.fna" % j)).write_bytes(fasta(ident, seq))
    return multi, single, records


def sketch(hg, path, out, *more):
    r = subprocess.run([hg.CLI_PATH, "sketch", "-p", str(path), "-o", str(out), "-s", "20", "-t", "2", *more], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return r.stdout


@pytest.mark.parametrize("more", [(), ("-D", "gpu", "-C", "false", "-k", "17", "--min_count", "2", "--pack_layout", "naive")])
def test_individual_equals_one_file_per_record(hg, dirs, tmp_path, more):
    multi, single, records = dirs
    out = sketch(hg, multi, tmp_path / "i.sketch", "--individual", *more)
    assert "Sketching 7 records of 2 files took" in out
    assert "Sketching 7 files took" in sketch(hg, single, tmp_path / "s.sketch", *more)
    got, want = hg.read_sketch_file(str(tmp_path / "i.sketch")), hg.read_sketch_file(str(tmp_path / "s.sketch"))
    assert len(got) == len(want) == 7
    assert [x["file_str"] for x in got] == [ident.decode() for ident, _ in records]  # the identifiers, in order, no path
    assert [x["file_str"] for x in want] == [str(single / ("r%02d.fna" % j)) for j in range(7)]
    for g, w in zip(got, want):
        assert [g[f] for f in FIELDS] == [w[f] for f in FIELDS]
        assert g["hv"].tobytes() == w["hv"].tobytes()
    # (the sketches are not all one and the same; under --min_count 2 only the record with the repeat keeps k-mers)
    assert len({x["hv"].tobytes() for x in got}) >= (2 if more else 5)


def test_min_length_drops_exactly_the_short_records(hg, dirs, tmp_path):
    multi, single, records = dirs
    sketch(hg, multi, tmp_path / "all.sketch", "--individual")
    out = sketch(hg, multi, tmp_path / "long.sketch", "--individual", "--min_length", "1000")
    assert "Sketching 4 records of 2 files took" in out and "3 records shorter than 1000 were left out" in out
    every, long = hg.read_sketch_file(str(tmp_path / "all.sketch")), hg.read_sketch_file(str(tmp_path / "long.sketch"))
    keep = [j for j, (_, seq) in enumerate(records) if len(seq) >= 1000]
    assert len(keep) == 4 and [x["file_str"] for x in long] == [records[j][0].decode() for j in keep]
    for x, j in zip(long, keep):
        assert x["hv"].tobytes() == every[j]["hv"].tobytes() and x["hv_norm_2"] == every[j]["hv_norm_2"]
    # --min_length 0 is the default
    sketch(hg, multi, tmp_path / "zero.sketch", "--individual", "--min_length=0")
    assert (tmp_path / "zero.sketch").read_bytes() == (tmp_path / "all.sketch").read_bytes()


def test_dist_prints_the_identifiers(hg, dirs, tmp_path):
    multi, single, records = dirs
    sk, tsv = tmp_path / "i.sketch", tmp_path / "i.tsv"
    sketch(hg, multi, sk, "--individual", "--min_length", "1000")
    r = subprocess.run([hg.CLI_PATH, "dist", "-r", str(sk), "-q", str(sk), "-o", str(tsv), "-a", "0"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    names = {line.split("\t")[0] for line in tsv.read_text().splitlines()} | {line.split("\t")[1] for line in tsv.read_text().splitlines()}
    assert names == {ident.decode() for ident, seq in records if len(seq) >= 1000}


def test_what_the_mode_refuses_in_a_file(hg, tmp_path):
    for name, text, words in (("noid", b">ok\nACGT\n> description only\nACGT\n", "record 2 has an empty identifier"),
                              ("fastq", b"@r1\nACGT\n+\nIIII\n", "sequence data before the first header")):
        d = tmp_path / name
        d.mkdir()
        (d / "x.fna").write_bytes(text)
        r = subprocess.run([hg.CLI_PATH, "sketch", "--individual", "-p", str(d), "-o", str(tmp_path / "x.sketch")], capture_output=True, text=True)
        assert r.returncode == 2 and r.stderr.startswith("error: " + str(d / "x.fna") + ": ") and words in r.stderr, r.stderr
