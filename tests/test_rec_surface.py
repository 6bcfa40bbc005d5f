"""libhypergen_rec.so and `hyper-gen sketch --individual`, the parts that need no GPU: include/hypergen_rec.h, the library's
exports and the Python mirror agree; the library borrows nothing from the test oracle and links the main one; hg_rec_split_host
-- one host thread's reading of the specification -- against tests/rec_ref.py on every text of tests/rec_cases.py and on the
seeded fuzz, the whole output buffer with its pads and a sentinel behind it; 'N' + sequence over the records is what
hg_read_merge_seq makes of the same file; the command line describes the two options in `sketch --help` only and rejects
what it must before a device is opened."""
import os
import re
import subprocess

import numpy as np
import pytest

import rec_cases
import rec_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "hypergen_rec.h")
FILL = 0xEE


@pytest.fixture(scope="module")
def hg():
    import hypergen_amd
    hypergen_amd.lib_rec()
    return hypergen_amd


@pytest.fixture(scope="module")
def texts(hg):
    B = hg.rec_block_bytes()
    return rec_cases.cases(B) + [("fuzz_%03d" % i, t) for i, t in enumerate(rec_cases.fuzz_texts(B))]


def exported(path):
    nm = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return [line.split()[-1] for line in nm.splitlines() if line.split()[-2] in ("T", "t", "W")]


def test_every_declared_symbol_is_exported_and_bound(hg):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(hg_rec_\w+)\s*\(", text)))
    assert declared == sorted(hg.REC_EXPORTS) and len(declared) == 9
    c_names = sorted(s for s in exported(hg.REC_LIB_PATH) if s.startswith("hg_rec_") and not s.startswith("_Z"))
    assert c_names == declared
    for name in declared:
        assert getattr(hg.lib_rec(), name).argtypes is not None, name
    # the other libraries' surfaces are what they were: nothing of this one went into them
    assert not [s for s in hg.EXPORTS + hg.AA_EXPORTS + hg.TX_EXPORTS if s.startswith("hg_rec_")]
    for path in (hg.LIB_PATH, hg.AA_LIB_PATH, hg.TX_LIB_PATH):
        assert not [s for s in exported(path) if "hg_rec_" in s]


def test_library_defines_no_oracle_symbol_and_links_the_main_library(hg):
    assert not [s for s in exported(hg.REC_LIB_PATH) if "orc_" in s]
    dyn = subprocess.run(["readelf", "-d", hg.REC_LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "libhypergen_hip.so" in dyn and "$ORIGIN" in dyn and "libz" in dyn


def test_record_entry_and_geometry(hg):
    assert hg.REC_DTYPE == rec_ref.REC_DTYPE and hg.REC_DTYPE.itemsize == 32
    B = hg.rec_block_bytes()
    assert B % 16 == 0 and B >= 1024
    assert len(hg.rec_kernel_names()) == len(set(hg.rec_kernel_names())) == 8


def same_split(got, text):
    """(status, n_recs, seq_bytes, recs, seq) of a splitter run with exact capacities against the reference"""
    st, n_recs, seq_bytes, recs, seq = got
    try:
        want = rec_ref.split(text)
    except rec_ref.SequenceBeforeHeader:
        return st == 7
    table, buf = rec_ref.layout(want)
    return (st == 0 and n_recs == len(want) and seq_bytes == buf.size and recs.size == table.size and seq.size == buf.size + 32
            and bool((recs == table).all()) and bool((seq[:buf.size] == buf).all()) and bool((seq[buf.size:] == FILL).all()))


def test_host_splitter_equals_the_reference_on_every_case(hg, texts):
    oks = errors = 0
    for name, text in texts:
        got = hg.rec_split_host(text, fill=FILL)
        assert same_split(got, text), name
        errors += got[0] == hg.ERR_IO
        oks += got[0] == hg.OK
    assert oks > 150 and errors > 20  # (both kinds of text are there in numbers)


def test_anchor_by_hand(hg):
    st, n_recs, seq_bytes, recs, seq = hg.rec_split_host(rec_cases.ANCHOR, fill=FILL)
    assert (st, n_recs, seq_bytes) == (0, 3, 20 + 8 + 12)
    assert recs["hdr_off"].tolist() == [0, 39, 53] and recs["hdr_len"].tolist() == [18, 5, 11] and recs["id_len"].tolist() == [4, 4, 4]
    assert recs["seq_off"].tolist() == [0, 20, 28] and recs["seq_len"].tolist() == [18, 6, 9]
    assert seq[:seq_bytes].tobytes() == b"ACGTACGTACGGTTAACCNN" + b"TTTTACNN" + b"GATTACAGANNN"
    assert rec_ref.identifiers(rec_cases.ANCHOR, rec_ref.split(rec_cases.ANCHOR)) == [b"seq1", b"seq2", b"seq3"]


def test_host_splitter_capacities_and_sentinels(hg):
    text = dict(rec_cases.cases(hg.rec_block_bytes()))["lengths_0_to_9"]
    table, buf = rec_ref.layout(rec_ref.split(text))
    for seq_cap, rec_cap in ((buf.size + 31, table.size), (buf.size + 32, table.size - 1), (0, 0), (7, 3)):
        st, n_recs, seq_bytes, recs, seq = hg.rec_split_host(text, seq_cap=seq_cap, rec_cap=rec_cap, fill=FILL)
        assert (st, n_recs, seq_bytes) == (hg.ERR_CAPACITY, table.size, buf.size), (seq_cap, rec_cap)
        assert seq.size == seq_cap and recs.size == rec_cap  # (what fits may have been written, nothing else exists)
    # room to spare: everything behind seq_bytes and behind n_recs entries stays as it was
    st, n_recs, seq_bytes, recs, seq = hg.rec_split_host(text, seq_cap=buf.size + 100, rec_cap=table.size + 2, fill=FILL)
    assert st == hg.OK and (seq[:buf.size] == buf).all() and (seq[buf.size:] == FILL).all()
    assert (recs[:n_recs] == table).all() and (recs[n_recs:].view(np.uint8) == FILL).all()
    import ctypes as C
    n = C.c_size_t(0)
    assert hg.lib_rec().hg_rec_split_host(None, 0, None, 0, None, 0, None, C.byref(n)) == hg.ERR_INVALID
    assert hg.lib_rec().hg_rec_split_host(None, 1 << 32, None, 0, None, 0, C.byref(n), C.byref(n)) == hg.ERR_UNSUPPORTED


def test_records_joined_with_n_are_what_read_merge_seq_returns(hg, texts, tmp_path):
    checked = 0
    for name, text in texts:
        st, n_recs, seq_bytes, recs, seq = hg.rec_split_host(text, fill=FILL)
        if st != hg.OK:
            continue
        path = tmp_path / "t.fna"
        path.write_bytes(text)
        joined = b"".join(b"N" + seq[int(r["seq_off"]):int(r["seq_off"] + r["seq_len"])].tobytes() for r in recs)
        assert joined == hg.read_merge_seq(str(path)).tobytes() == rec_ref.merged(rec_ref.split(text)), name
        checked += 1
    assert checked > 150


# ---- command line ------------------------------------------------------------------------------------------------------------

def run_cli(hg, *args):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")  # (no device: all of this is decided before one is opened)
    return subprocess.run([hg.CLI_PATH, *args], capture_output=True, text=True, env=env)


def test_sketch_help_describes_both_options_behind_the_translate_text(hg):
    general = run_cli(hg, "--help")
    assert general.returncode == 0 and "--individual" not in general.stdout and "--min_length" not in general.stdout
    r = run_cli(hg, "sketch", "--help")
    assert r.returncode == 0 and r.stdout.startswith(general.stdout)
    paras = r.stdout[len(general.stdout):].split("\n\n")
    assert len(paras) == 2 and paras[1].startswith("sketch --translate:") and paras[1].endswith("\n")
    at = paras[1].index("\nsketch --individual [--min_length N]:")
    assert "--individual" not in paras[1][:at] and "--individual" not in paras[0]
    for word in ("one sketch per FASTA record", "Mash -i", "identifier", "--min_length N [0]", "--alphabet protein", "--translate",
                 "--shards", "4 GiB", "first visible GPU"):
        assert word in paras[1][at:], word
    for mode in ("dist", "search", "cluster"):
        out = run_cli(hg, mode, "--help").stdout
        assert "--individual" not in out and "--min_length" not in out


CLI_ERRORS = [
    (("dist", "--individual"), "error: --individual is not supported by dist: it splits the FASTA files sketch reads into their records\n"),
    (("search", "--individual"), "error: --individual is not supported by search: it splits the FASTA files sketch reads into their records\n"),
    (("cluster", "--individual"), "error: --individual is not supported by cluster: it splits the FASTA files sketch reads into their records\n"),
    (("dist", "--min_length", "5"), "error: --min_length is not supported by dist: it belongs to sketch --individual\n"),
    (("sketch", "--min_length", "5"),
     "error: --min_length needs --individual: without it sketch makes one sketch per file, whatever its length\n"),
    (("sketch", "--min_length=0"),
     "error: --min_length needs --individual: without it sketch makes one sketch per file, whatever its length\n"),
    (("sketch", "--individual", "--alphabet", "protein"),
     "error: --individual is not supported with --alphabet protein: protein input is sketched one file at a time\n"),
    (("sketch", "--translate", "--individual"),
     "error: --individual is not supported with --translate: translated input is sketched one file at a time\n"),
    (("sketch", "--individual", "--shards", "2"),
     "error: --shards is not supported with --individual: the records are sketched on the first visible GPU\n"),
    (("sketch", "--individual=1"), "error: unexpected argument '--individual=1'\n"),
    (("sketch", "--individual", "--min_length", "x"), "error: invalid value 'x' for '--min_length'\n"),
    (("sketch", "--individual", "--min_length"), "error: a value is required for '--min_length'\n"),
    # what is not rejected goes on to the required arguments, as ever
    (("sketch", "--individual", "--min_length", "1000", "--min_count", "2", "-k", "255"),
     "error: the following required arguments were not provided: --path --out\n"),
    (("sketch", "--individual"), "error: the following required arguments were not provided: --path --out\n"),
]


@pytest.mark.parametrize("args,stderr", CLI_ERRORS)
def test_cli_error_lines(hg, args, stderr):
    r = run_cli(hg, *args)
    assert (r.returncode, r.stdout, r.stderr) == (2, "", stderr)
