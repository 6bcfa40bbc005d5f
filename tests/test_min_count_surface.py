"""hg_sketch_params.min_count on the CPU: the header, the library's exports and the Python mirror agree on the new entry point and
on the field that took `reserved`'s place; the command line lists the flag and rejects what it must before a device is opened;
and the motivation, through the oracle alone: the ANI between a 30x read set and its genome under min_count = 1, 2, 3."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import min_count_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "hypergen.h")


@pytest.fixture(scope="module")
def hg():
    import hypergen_amd
    hypergen_amd.lib()
    return hypergen_amd


def test_entry_point_is_declared_exported_and_bound(hg):
    text = open(HEADER).read()
    assert re.search(r"hg_status\s+hg_kmer_hash_sample_min_count\s*\(", text)
    nm = subprocess.run(["nm", "-D", "--defined-only", hg.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT hg_kmer_hash_sample_min_count$", nm, re.M)
    assert "hg_kmer_hash_sample_min_count" in hg.EXPORTS
    assert hg.lib().hg_kmer_hash_sample_min_count.argtypes is not None


class _OldParams(C.Structure):  # hg_sketch_params as it was: the last field named `reserved`
    _fields_ = [("ksize", C.c_uint32), ("canonical", C.c_uint32), ("scaled", C.c_uint64), ("seed", C.c_uint64),
                ("hv_d", C.c_uint32), ("hv_layout", C.c_uint32), ("norm_mode", C.c_uint32), ("reserved", C.c_uint32)]


def test_min_count_takes_the_place_of_reserved(hg):
    text = open(HEADER).read()
    body = re.search(r"typedef struct \{([^}]*)\} hg_sketch_params;", text).group(1)
    fields = re.findall(r"^\s*(uint\d+_t)\s+(\w+);", body, re.M)
    assert fields[-1] == ("uint32_t", "min_count") and "reserved" not in [f for _, f in fields]
    assert [f for _, f in fields] == [f for f, _ in hg.SketchParams._fields_]
    assert hg.SketchParams.min_count.offset == _OldParams.reserved.offset == 36
    assert C.sizeof(hg.SketchParams) == C.sizeof(_OldParams) == 40
    p = hg.default_params()
    assert p.min_count == 0  # hg_sketch_params_default keeps writing 0: every sampled k-mer
    assert hg.default_params(min_count=3, scaled=200).min_count == 3


def run_cli(hg, *args):
    # (no device can be opened: whatever is rejected here is rejected before one is asked for)
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    return subprocess.run([hg.CLI_PATH, *args], capture_output=True, text=True, env=env)


def test_cli_lists_and_checks_the_flag(hg, tmp_path):
    r = run_cli(hg, "--help")
    ext = r.stdout[r.stdout.index("extensions:"):]
    assert r.returncode == 0 and "--min_count" in ext
    for bad in ("0", "two", "-1", ""):
        r = run_cli(hg, "sketch", "-p", str(tmp_path), "-o", str(tmp_path / "o.sketch"), "--min_count", bad)
        assert r.returncode != 0 and "invalid value '%s' for '--min_count'" % bad in r.stderr, (bad, r.stderr)
    for mode in ("dist", "search", "cluster"):
        r = run_cli(hg, mode, "-r", "a.sketch", "-q", "b.sketch", "-p", "a.sketch", "-o", str(tmp_path / "o"), "--min_count", "2")
        assert r.returncode != 0 and "--min_count is not supported by %s" % mode in r.stderr, (mode, r.stderr)


def test_read_set_needs_the_filter(orc):
    """the table of the README: 300 kbp, 30x of 150-base reads, 1 % substitutions, both strands; k = 21, scaled = 200, D = 4096"""
    reads, genome = ref.read_set()
    raw = orc.kmer_hash_sample(reads, 21, 200, unique=False)
    gset = orc.kmer_hash_sample(genome, 21, 200)
    vals, counts = np.unique(raw, return_counts=True)
    assert (raw.size, int((counts == 1).sum()), int(counts.max()), gset.size) == (37_535, 6_899, 37, 1_431)
    ghv = orc.encode_hv(gset)
    gn2 = orc.hv_norm2(ghv)
    ani = {}
    for m in (1, 2, 3, 4):
        k = ref.kept(raw, m)
        hv = orc.encode_hv(k)
        dot = int(hv.astype(np.int64) @ ghv.astype(np.int64))
        ani[m] = orc.ani_from_dot(dot, gn2, orc.hv_norm2(hv), 21)
        print("min_count %d: %d hashes, ANI %.3f" % (m, k.size, ani[m]))
    assert [ref.kept(raw, m).size for m in (1, 2, 3, 4)] == [8_570, 1_671, 1_433, 1_431]
    assert ani[1] < 96 < 99 < ani[2] < ani[3]
    assert np.isin(gset, ref.kept(raw, 4)).all()
