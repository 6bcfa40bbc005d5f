"""libhypergen_aa.so and `hyper-gen sketch --alphabet`, the parts that need no GPU: include/hypergen_aa.h, the library's exports
and the Python mirror agree; the companion library borrows nothing from the test oracle; hg_aa_read_fasta against a Python parse;
the command line names the flag in `sketch --help` and rejects what it must before a device is opened."""
import gzip
import os
import re
import subprocess

import pytest

import aa_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "hypergen_aa.h")


@pytest.fixture(scope="module")
def hg():
    import hypergen_amd
    hypergen_amd.lib_aa()
    return hypergen_amd


def exported(path):
    nm = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return [line.split()[-1] for line in nm.splitlines() if line.split()[-2] in ("T", "t", "W")]


def test_every_declared_symbol_is_exported_and_bound(hg):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(hg_aa_\w+)\s*\(", text)))
    assert declared == sorted(hg.AA_EXPORTS) and len(declared) == 7
    c_names = sorted(s for s in exported(hg.AA_LIB_PATH) if s.startswith("hg_aa_") and not s.startswith("_Z"))
    assert c_names == declared
    for name in declared:
        assert getattr(hg.lib_aa(), name).argtypes is not None, name
    # the nucleotide library's surface is what it was: nothing of this one went into it
    assert not [s for s in hg.EXPORTS if s.startswith("hg_aa_")]
    assert not [s for s in exported(hg.LIB_PATH) if "hg_aa_" in s]


def test_library_defines_no_oracle_symbol_and_links_the_main_library(hg):
    assert not [s for s in exported(hg.AA_LIB_PATH) if "orc_" in s]
    dyn = subprocess.run(["readelf", "-d", hg.AA_LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "libhypergen_hip.so" in dyn and "$ORIGIN" in dyn


def test_kernel_names_and_geometry(hg):
    for k in range(1, 33):
        assert hg.aa_kernel_name(k) == "aa_kmer_sample_kernel<%d>" % ((k + 7) // 8)
        assert hg.aa_item_starts(k) % 4 == 0 and hg.aa_item_starts(k) > hg.aa_tile_starts()
    assert hg.aa_kernel_name(0) == "" and hg.aa_kernel_name(33) == "" and hg.aa_item_starts(33) == 0
    assert hg.aa_tile_starts() % 4 == 0


FASTA_CASES = {
    "multi": b">p1 first\nMKVLAAGIW\nRTYPLDE\n>p2\nQSNHFC\n",
    "crlf": b">p1\r\nMKVL\r\nAAGI\r\n>p2\r\nWRTY\r\n",
    "blank_lines": b"\n>p1\n\nMKVL\n\n\nAAGI\n>p2\n\n",
    "lower_and_mixed": b">p1\nmkvlAAgiw\n>p2\nacdefghiklmnpqrstvwy\n",
    "empty_record": b">p1\n>p2\nMKVL\n>p3\n",
    "no_trailing_newline": b">p1\nMKVL\n>p2\nAAGI",
    "blanks_and_tabs": b">p1 a\tb\nMK VL\tAA \n  GI\n",
    "stop_and_unknown": b">p1\nMKVL*\n>p2\nAXBZ-U.J\n",
    "no_header": b"MKVL\nAAGI\n",
    "gt_inside_a_line": b">p1\nMK>VL\n",
    "empty_file": b"",
}


@pytest.mark.parametrize("name", sorted(FASTA_CASES))
@pytest.mark.parametrize("gz", [False, True])
def test_read_fasta_equals_a_python_parse(hg, tmp_path, name, gz):
    data = FASTA_CASES[name]
    path = tmp_path / ("x.faa.gz" if gz else "x.faa")
    path.write_bytes(gzip.compress(data) if gz else data)
    got = hg.aa_read_fasta(str(path)).tobytes()
    assert got == aa_ref.parse_fasta(data)
    if name == "multi":
        assert got == b"*MKVLAAGIWRTYPLDE*QSNHFC"
    if name == "empty_record":
        assert got == b"**MKVL*"


def test_read_fasta_long_file_and_missing_file(hg, tmp_path):
    # longer than one read block, a record boundary wherever the blocks fall
    rec = b">protein\n" + b"ACDEFGHIKLMNPQRSTVWY" * 3 + b"\n" + b"MKV\n"
    data = rec * 40_000
    (tmp_path / "big.faa").write_bytes(data)
    assert hg.aa_read_fasta(str(tmp_path / "big.faa")).tobytes() == aa_ref.parse_fasta(data)
    with pytest.raises(hg.HgError) as e:
        hg.aa_read_fasta(str(tmp_path / "none.faa"))
    assert e.value.status == hg.ERR_IO


def run_cli(hg, *args):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")  # (no device: all of this is decided before one is opened)
    return subprocess.run([hg.CLI_PATH, *args], capture_output=True, text=True, env=env)


def test_sketch_help_is_the_general_help_and_one_paragraph(hg):
    general = run_cli(hg, "--help")
    assert general.returncode == 0 and "--alphabet" not in general.stdout
    for flag in ("--help", "-h"):
        r = run_cli(hg, "sketch", flag)
        assert r.returncode == 0 and r.stdout.startswith(general.stdout)
        para = r.stdout[len(general.stdout):]
        assert para.startswith("\nsketch --alphabet dna|protein [dna]:") and "cannot tell a protein sketch file from a nucleotide one" in para
    for mode in ("dist", "cluster"):
        assert "--alphabet" not in run_cli(hg, mode, "--help").stdout


CLI_ERRORS = [
    (("sketch", "--alphabet", "rna"), "error: invalid value 'rna' for '--alphabet' (dna | protein)\n"),
    (("sketch", "--alphabet", ""), "error: invalid value '' for '--alphabet' (dna | protein)\n"),
    (("dist", "--alphabet", "protein"), "error: --alphabet is not supported by dist: it names the alphabet of the sequences sketch reads\n"),
    (("search", "--alphabet", "dna"), "error: --alphabet is not supported by search: it names the alphabet of the sequences sketch reads\n"),
    (("cluster", "--alphabet=protein",), "error: --alphabet is not supported by cluster: it names the alphabet of the sequences sketch reads\n"),
    (("sketch", "--alphabet", "protein", "--min_count", "2"),
     "error: --min_count is not supported with --alphabet protein: amino-acid k-mers are sketched without the count filter\n"),
    (("sketch", "--alphabet", "protein", "--shards", "2"),
     "error: --shards is not supported with --alphabet protein: protein input is sketched on the first visible GPU\n"),
    (("sketch", "--alphabet", "protein", "-k", "33"),
     "error: invalid value '33' for '--ksize': --alphabet protein takes k-mers of 1 to 32 residues\n"),
    # what is not rejected goes on to the required arguments, as ever
    (("sketch", "--alphabet", "protein", "--min_count", "1", "-k", "32"), "error: the following required arguments were not provided: --path --out\n"),
    (("sketch", "--alphabet", "dna", "--min_count", "2", "--shards", "2", "-k", "33"),
     "error: the following required arguments were not provided: --path --out\n"),
    (("sketch", "--alphabet"), "error: a value is required for '--alphabet'\n"),
]


@pytest.mark.parametrize("args,stderr", CLI_ERRORS)
def test_cli_error_lines(hg, args, stderr):
    r = run_cli(hg, *args)
    assert (r.returncode, r.stdout, r.stderr) == (2, "", stderr)
