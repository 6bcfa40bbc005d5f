"""hg_ani_pairs{,_dev}, `dist --columns` and `dist --pairs`: what can be checked without a device -- the declarations, the
exports, the Python surface, the command line's argument errors, and the reference the GPU tests compare with."""
import os
import re
import subprocess

import numpy as np
import pytest

import ani_pairs_ref as ap
import containment_ref as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def hg():
    import hypergen_amd
    hypergen_amd.lib()
    return hypergen_amd


def cli(hg, *args):
    return subprocess.run([hg.CLI_PATH, *args], capture_output=True, text=True, timeout=60)


def test_header_declares_the_entry_points_and_constants():
    hdr = open(os.path.join(ROOT, "include", "hypergen.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"\bhg_status\s+hg_ani_pairs_dev\s*\(", code) and re.search(r"\bhg_status\s+hg_ani_pairs\s*\(", code)
    want = {"HG_PAIRS_MASH": 1, "HG_PAIRS_CONTAINMENT": 2, "HG_PAIRS_MAX_CONTAINMENT": 4, "HG_PAIRS_CONTAINMENT_REF": 8,
            "HG_PAIRS_EMPTY": 0xFFFFFFFF}
    for name, value in want.items():
        m = re.search(r"#define\s+%s\s+(0x[0-9A-Fa-f]+|\d+)u\b" % name, code)
        assert m and int(m.group(1), 0) == value, name
    assert "hg_ani_pairs" in hdr[hdr.index("hg_ctx_set_ani_metric: host-side state"): hdr.index("#define HG_ANI_MASH")]  # listed as independent of the metric


def test_symbols_are_exported_and_resolve(hg):
    L = hg.lib()
    for name in ("hg_ani_pairs_dev", "hg_ani_pairs"):
        assert name in hg.EXPORTS and hasattr(L, name)
        assert len(getattr(L, name).argtypes) == 14
    nm = subprocess.run(["nm", "-C", hg.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r"::ani_pairs_kernel\(", nm)


def test_python_surface(hg):
    assert callable(hg.Context.ani_pairs) and callable(hg.Context.ani_pairs_dev)
    assert (hg.PAIRS_MASH, hg.PAIRS_CONTAINMENT, hg.PAIRS_MAX_CONTAINMENT, hg.PAIRS_CONTAINMENT_REF) == ap.BITS == (1, 2, 4, 8)
    assert hg.PAIRS_EMPTY == ap.EMPTY == 0xFFFFFFFF


def test_help_names_the_flags(hg):
    out = cli(hg, "--help").stdout
    assert "--columns" in out and "--pairs" in out and "containment_ref" in out


@pytest.mark.parametrize("value", ["nonsense", "", "mash,mash", "mash,,containment", "mash,Containment", ","])
def test_bad_columns_fail_in_argument_parsing(hg, tmp_path, value):
    """no sketch file exists and no device is opened: the value is refused first"""
    r = cli(hg, "dist", "-r", str(tmp_path / "a.sketch"), "-q", str(tmp_path / "b.sketch"), "-o", str(tmp_path / "o.tsv"), "--columns", value)
    assert r.returncode != 0 and ("'%s'" % value) in r.stderr and "--columns" in r.stderr, r.stderr
    assert "Loading sketch" not in r.stdout and not (tmp_path / "o.tsv").exists()


@pytest.mark.parametrize("mode", ["sketch", "search", "cluster"])
@pytest.mark.parametrize("flag", [("--columns", "mash"), ("--pairs", "list.tsv")])
def test_other_subcommands_refuse_the_flags(hg, tmp_path, mode, flag):
    files = ["-p", str(tmp_path), "-o", str(tmp_path / "o")] if mode != "search" else ["-r", "a", "-q", "b", "-o", str(tmp_path / "o")]
    r = cli(hg, mode, *files, *flag)
    assert r.returncode != 0 and ("%s is not supported by %s" % (flag[0], mode)) in r.stderr, r.stderr


@pytest.mark.parametrize("flag", [("--columns", "mash"), ("--pairs", "list.tsv")])
def test_shards_are_refused_with_the_flags(hg, tmp_path, flag):
    r = cli(hg, "dist", "-r", "a", "-q", "b", "-o", str(tmp_path / "o"), "--shards", "2", *flag)
    assert r.returncode != 0 and ("%s is not supported with --shards" % flag[0]) in r.stderr, r.stderr


def test_reference_columns_by_hand(orc):
    """ani_pairs_ref against containment_ref.ani_ref and values worked out by hand (k = 21)"""
    k = 21
    u32 = lambda a: np.asarray(a, np.float32).view(np.uint32)

    def row(dot, nr, nq):
        return ap.columns(orc, ap.ALL, [dot], [nr], [nq], k)[0]

    # equal norms: x = dot / n in all four; 1 + ln(0.5) / 21 = 0.966993...  The Mash form reaches x = 0.5 through J = 1/3,
    # 1 / J, + 1 and 2 / inner (four roundings, relative 2^-24 each): two ulp of 96.7 (2^-17) bound the difference
    v = row(500, 1000, 1000)
    assert u32(v[1]) == u32(v[2]) == u32(v[3]) and abs(float(v[1]) - 96.69934) < 1e-4
    assert abs(float(v[0]) - float(v[1])) <= 2 * 2.0 ** -17
    # dot <= 0: 0 in every column
    assert (u32(row(0, 100, 100)) == 0).all() and (u32(row(-5, 100, 100)) == 0).all()
    # zero denominators: 0 / 0 -> NaN -> 0; x / 0 -> +inf -> 100; and 0 / n -> ln(0) = -inf -> 0
    assert (u32(row(0, 0, 0)) == 0).all()
    v = row(0, 5, 0)
    assert (u32(v) == 0).all()
    v = row(5, 0, 3)  # containment: 5 / 3 > 1 -> 100; containment_ref: 5 / 0 -> 100; max containment: 5 / 0 -> 100
    assert (v[1:] == np.float32(100.0)).all()
    # dot above the denominator: 100
    assert (row(200, 100, 100)[1:] == np.float32(100.0)).all()
    # direction: the reference is the small side (nr = 50), the query the large one (nq = 100), dot = 40
    v = row(40, 50, 100)
    want_q = np.float32(100.0) * (np.float32(1.0) + orc.logf_array(np.float32([0.4]))[0] / np.float32(k))
    want_r = np.float32(100.0) * (np.float32(1.0) + orc.logf_array(np.float32([0.8]))[0] / np.float32(k))
    assert u32(v[1]) == u32(want_q) and u32(v[3]) == u32(want_r) and u32(v[2]) == u32(v[3]) and v[1] < v[3]
    assert abs(float(v[1]) - 95.63670) < 1e-4 and abs(float(v[3]) - 98.93741) < 1e-4
    # the layout: ascending bits, and each column is ani_ref's
    dot, nr, nq = np.int32([40, 7, 500]), np.int32([50, 9, 1000]), np.int32([100, 8, 700])
    got = ap.columns(orc, ap.CONTAINMENT | ap.CONTAINMENT_REF, dot, nr, nq, k)
    assert got.shape == (3, 2)
    assert (u32(got[:, 0]) == u32(cr.ani_ref(orc, dot, nr, nq, k, cr.CONTAINMENT))).all()
    assert (u32(got[:, 1]) == u32(cr.ani_ref(orc, dot, nq, nr, k, cr.CONTAINMENT))).all()
    assert (u32(ap.columns(orc, ap.MASH, dot, nr, nq, k)[:, 0]) == u32(cr.ani_ref(orc, dot, nr, nq, k, cr.MASH))).all()
    assert ap.place(ap.ALL, ap.CONTAINMENT_REF) == 3 and ap.place(10, ap.CONTAINMENT_REF) == 1 and ap.place(10, ap.CONTAINMENT) == 0
