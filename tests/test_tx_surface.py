"""libhypergen_tx.so and `hyper-gen sketch --translate`, the parts that need no GPU: include/hypergen_tx.h, the library's exports
and the Python mirror agree; the companion library borrows nothing from the test oracle; hg_tx_translate_frame -- the host's run of
the classification and codon functions the kernel fills its tables from -- against tests/tx_ref.py; the command line describes the
switch in `sketch --help` and rejects what it must before a device is opened."""
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import tx_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "hypergen_tx.h")
ANCHOR = b"ATGGCCATTGTAATGGGCCGCTGAAAGGGTGCCCGATAG"


@pytest.fixture(scope="module")
def hg():
    import hypergen_amd
    hypergen_amd.lib_tx()
    return hypergen_amd


def exported(path):
    nm = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return [line.split()[-1] for line in nm.splitlines() if line.split()[-2] in ("T", "t", "W")]


def test_every_declared_symbol_is_exported_and_bound(hg):
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(hg_tx_\w+)\s*\(", text)))
    assert declared == sorted(hg.TX_EXPORTS) and len(declared) == 9
    c_names = sorted(s for s in exported(hg.TX_LIB_PATH) if s.startswith("hg_tx_") and not s.startswith("_Z"))
    assert c_names == declared
    for name in declared:
        assert getattr(hg.lib_tx(), name).argtypes is not None, name
    # the other libraries' surfaces are what they were: nothing of this one went into them
    assert not [s for s in hg.EXPORTS + hg.AA_EXPORTS if s.startswith("hg_tx_")]
    for path in (hg.LIB_PATH, hg.AA_LIB_PATH):
        assert not [s for s in exported(path) if "hg_tx_" in s]


def test_library_defines_no_oracle_symbol_and_links_the_main_library(hg):
    assert not [s for s in exported(hg.TX_LIB_PATH) if "orc_" in s]
    dyn = subprocess.run(["readelf", "-d", hg.TX_LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "libhypergen_hip.so" in dyn and "$ORIGIN" in dyn


def test_kernel_names_and_geometry(hg):
    for k in range(1, 33):
        assert hg.tx_kernel_name(k) == "tx_kmer_sample_kernel<%d>" % ((k + 7) // 8)
        assert hg.tx_item_starts(k) % 4 == 0 and hg.tx_item_starts(k) > hg.tx_tile_starts()
        assert hg.tx_item_starts(k) == hg.aa_item_starts(k)  # the plan's, whatever the hook
    assert hg.tx_kernel_name(0) == "" and hg.tx_kernel_name(33) == "" and hg.tx_item_starts(33) == 0 and hg.tx_item_starts(0) == 0
    assert hg.tx_tile_starts() % 4 == 0 and hg.tx_tile_starts() > 3 * 32


# ---- the plan of a translated batch ------------------------------------------------------------------------------------------

def test_plan_is_sized_for_windows_of_3k_bytes_and_two_kmers_per_start(hg):
    """hg_tx_plan_describe against the rule of include/hypergen_tx.h, and against the nucleotide plan of the same lengths
    (hg_sketch_plan_describe: windows of k bytes, one k-mer per start) -- a dense translated call needs no regrown hit region"""
    import ctypes as C
    k = 9
    lens = [0, 26, 27, 28, 500, 6000, 30_000, 1_500_000]
    I = hg.tx_item_starts(k)

    def rounded(cap):  # a region beyond the one-workgroup sort is a power of two
        return cap if cap <= 8192 else 1 << (cap - 1).bit_length()

    for scaled in (1, 2, 40, 1500):
        for n in lens:
            d = hg.tx_plan_describe([n], k, scaled)
            starts = max(n - 3 * k + 1, 0)
            expect = 2 * starts // scaled
            cap = max(min(2 * expect + 1024, 2 * starts), 1)
            assert d["items"] == -(-starts // I) and d["item_starts"] == I, (scaled, n)
            assert d["max_cap"] == d["min_cap"] == d["slots"] == rounded(cap) >= min(2 * starts, cap), (scaled, n, d)
            assert d["max_expect"] == expect
        d = hg.tx_plan_describe(lens, k, scaled)
        assert d["items"] == sum(-(-max(n - 26, 0) // I) for n in lens) and d["min_cap"] == 1
    # dense: every window of both strands has a slot, which the plan for one k-mer per start does not give
    for n in (6000, 30_000):
        d = hg.tx_plan_describe([n], k, 1)
        assert d["min_cap"] >= 2 * (n - 26)
        counts = (C.c_uint64 * 6)()
        off, ln = (C.c_uint64 * 1)(0), (C.c_uint64 * 1)(n)
        assert hg.lib().hg_sketch_plan_describe(off, ln, 1, k, C.c_uint64(1), counts, None, 0) == hg.OK
        assert counts[3] < 2 * (n - 26) <= d["min_cap"]  # (the nucleotide plan's largest region: n - k + 1 k-mers, rounded)
    with pytest.raises(hg.HgError):
        hg.tx_plan_describe([100], 33, 1)
    with pytest.raises(hg.HgError):
        hg.tx_plan_describe([100], 9, 0)


# ---- hg_tx_translate_frame ---------------------------------------------------------------------------------------------------

def six(hg, s):
    return [hg.tx_translate_frame(s, f) for f in range(6)]


def test_the_anchor(hg):
    got = six(hg, ANCHOR)
    assert got[0] == b"MAIVMGR*KGAR*"
    assert got == tx_ref.frames(ANCHOR)
    assert [len(g) for g in got] == [13, 12, 12, 13, 12, 12]


def test_all_64_codons_in_three_cases(hg):
    codons = ["".join(c) for c in itertools.product("TCAG", repeat=3)]
    upper = "".join(codons).encode()
    assert hg.tx_translate_frame(upper, 0) == tx_ref.CODONS.encode()
    mixed = bytes(b | 0x20 if i % 2 else b for i, b in enumerate(upper))
    for s in (upper, upper.lower(), mixed, mixed.swapcase()):
        assert six(hg, s) == tx_ref.frames(s)
        assert hg.tx_translate_frame(s, 0) == tx_ref.CODONS.encode()
    # ... and on the other strand: the reverse complement of the codon list, read in frame 3, is the list backwards
    rc = tx_ref.revcomp(upper)
    assert hg.tx_translate_frame(rc, 3) == tx_ref.CODONS.encode()


def test_every_byte_value_at_each_codon_position(hg):
    bases = set(b"ACGTacgt")
    for pos in range(3):
        for v in range(256):
            for ctx_bases in (b"AC", b"gt", b"Tg"):
                codon = bytearray(ctx_bases[:1] * 3)
                codon[(pos + 1) % 3] = ctx_bases[1]
                codon[pos] = v
                s = b"ATG" + bytes(codon) + b"GCC"
                got = six(hg, s)
                assert got == tx_ref.frames(s), (pos, v)
                assert (got[0][1:2] == b"X") == (v not in bases)
                assert (got[3][1:2] == b"X") == (v not in bases)  # a non-base stays one at its mirrored place


def test_short_sequences_and_every_frame(hg):
    rng = np.random.default_rng(3)
    for n in range(0, 9):
        for _ in range(4):
            s = rng.choice(np.frombuffer(b"ACGTacgtN", np.uint8), n).tobytes()
            got = six(hg, s)
            assert got == tx_ref.frames(s), s
            assert [len(g) for g in got] == [max(n - f, 0) // 3 for f in (0, 1, 2, 0, 1, 2)]


def test_frames_3_to_5_are_frames_0_to_2_of_the_reverse_complement(hg):
    rng = np.random.default_rng(4)
    for n in (37, 38, 39, 1000, 1001, 1002):
        s = rng.choice(np.frombuffer(b"ACGTacgtNRYn-", np.uint8), n, p=[.2, .2, .2, .2, .04, .04, .04, .03, .01, .01, .01, .01, .01]).tobytes()
        rc = tx_ref.revcomp(s)
        got, got_rc = six(hg, s), six(hg, rc)
        assert got == tx_ref.frames(s)
        assert got[3:] == got_rc[:3] and got[:3] == got_rc[3:]


def test_translate_frame_statuses(hg):
    import ctypes as C
    L = hg.lib_tx()
    a = np.frombuffer(ANCHOR, np.uint8)
    out, n = np.zeros(64, np.uint8), C.c_size_t(0)
    assert L.hg_tx_translate_frame(a.ctypes.data, a.size, 6, out.ctypes.data, 64, C.byref(n)) == hg.ERR_INVALID
    assert L.hg_tx_translate_frame(a.ctypes.data, a.size, 0, out.ctypes.data, 12, C.byref(n)) == hg.ERR_CAPACITY and n.value == 13
    assert L.hg_tx_translate_frame(a.ctypes.data, a.size, 0, out.ctypes.data, 13, C.byref(n)) == hg.OK and n.value == 13
    assert L.hg_tx_translate_frame(None, 0, 5, None, 0, C.byref(n)) == hg.OK and n.value == 0
    assert L.hg_tx_translate_frame(a.ctypes.data, a.size, 0, out.ctypes.data, 64, None) == hg.ERR_INVALID


# ---- command line ------------------------------------------------------------------------------------------------------------

def run_cli(hg, *args):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")  # (no device: all of this is decided before one is opened)
    return subprocess.run([hg.CLI_PATH, *args], capture_output=True, text=True, env=env)


def test_sketch_help_gains_a_second_paragraph(hg):
    general = run_cli(hg, "--help")
    assert general.returncode == 0 and "--translate" not in general.stdout
    for flag in ("--help", "-h"):
        r = run_cli(hg, "sketch", flag)
        assert r.returncode == 0 and r.stdout.startswith(general.stdout)
        paras = r.stdout[len(general.stdout):].split("\n\n")
        assert len(paras) == 2
        assert paras[0].startswith("\nsketch --alphabet dna|protein [dna]:") and "--translate" not in paras[0]
        assert paras[0].endswith("dna is what sketch does without the option.")
        assert paras[1].startswith("sketch --translate:") and paras[1].endswith("\n")
        for word in ("six reading frames", "NCBI table 1", "containment", "--alphabet protein", "--min_count", "--shards", "-k above 32"):
            assert word in paras[1], word
    for mode in ("dist", "cluster"):
        assert "--translate" not in run_cli(hg, mode, "--help").stdout


CLI_ERRORS = [
    (("dist", "--translate"), "error: --translate is not supported by dist: it translates the nucleotide sequences sketch reads\n"),
    (("search", "--translate"), "error: --translate is not supported by search: it translates the nucleotide sequences sketch reads\n"),
    (("cluster", "--translate"), "error: --translate is not supported by cluster: it translates the nucleotide sequences sketch reads\n"),
    (("sketch", "--translate", "--alphabet", "protein"),
     "error: --translate is not supported with --alphabet protein: protein input is not translated\n"),
    (("sketch", "--alphabet=protein", "--translate", "--min_count", "2"),
     "error: --translate is not supported with --alphabet protein: protein input is not translated\n"),
    (("sketch", "--translate", "--min_count", "2"),
     "error: --min_count is not supported with --translate: amino-acid k-mers are sketched without the count filter\n"),
    (("sketch", "--translate", "--shards", "2"),
     "error: --shards is not supported with --translate: translated input is sketched on the first visible GPU\n"),
    (("sketch", "--translate", "-k", "33"), "error: invalid value '33' for '--ksize': --translate takes k-mers of 1 to 32 residues\n"),
    (("sketch", "--translate=1"), "error: unexpected argument '--translate=1'\n"),
    # what is not rejected goes on to the required arguments, as ever
    (("sketch", "--translate", "--alphabet", "dna", "--min_count", "1", "-k", "32"),
     "error: the following required arguments were not provided: --path --out\n"),
    (("sketch", "--translate"), "error: the following required arguments were not provided: --path --out\n"),
]


@pytest.mark.parametrize("args,stderr", CLI_ERRORS)
def test_cli_error_lines(hg, args, stderr):
    r = run_cli(hg, *args)
    assert (r.returncode, r.stdout, r.stderr) == (2, "", stderr)
