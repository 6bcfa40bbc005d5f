"""The containment ANI metrics, the parts that need no GPU: the C ABI's declarations and exports, the Python mirror, the
command line's surface (help, what it rejects before a device is opened), and the formula of tests/containment_ref.py
against the oracle's Mash-style ANI where the two must agree."""
import os
import re
import subprocess

import numpy as np
import pytest

import containment_ref as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("hg_ctx_set_ani_metric", "hg_ctx_ani_metric", "hg_multi_set_ani_metric")


@pytest.fixture(scope="module")
def hg():
    import hypergen_amd
    hypergen_amd.lib()
    return hypergen_amd


def run(hg, *args):
    return subprocess.run([hg.CLI_PATH] + list(args), capture_output=True, text=True, timeout=60)


def test_metric_symbols_declared_exported_and_mirrored(hg):
    hdr_full = open(os.path.join(ROOT, "include", "hypergen.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr_full, flags=re.S)
    nm = subprocess.run(["nm", "-D", "--defined-only", hg.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r"\bT (hg_\w+)", nm))
    for name in NAMES:
        assert re.search(r"\b(hg_status|int) %s\(" % name, hdr), name
        assert name in exported, name
        assert name in hg.EXPORTS, name
    for name, v in (("HG_ANI_MASH", 0), ("HG_ANI_CONTAINMENT", 1), ("HG_ANI_MAX_CONTAINMENT", 2)):
        assert re.search(r"#define %s %d\b" % (name, v), hdr), name
        assert getattr(hg, name[3:]) == v
    assert callable(hg.Context.set_ani_metric) and callable(hg.Context.ani_metric) and callable(hg.Multi.set_ani_metric)


def test_help_lists_ani_metric(hg):
    r = run(hg, "--help")
    assert r.returncode == 0
    assert "--ani_metric mash|containment|max_containment [mash]" in r.stdout


def test_unknown_metric_rejected_before_any_device(hg, tmp_path):
    out = tmp_path / "out.tsv"
    r = run(hg, "dist", "-r", str(tmp_path / "missing.sketch"), "-q", str(tmp_path / "missing2.sketch"), "-o", str(out),
            "--ani_metric", "bogus")
    assert r.returncode != 0
    assert "invalid value 'bogus' for '--ani_metric'" in r.stderr
    assert not out.exists()


def test_cluster_rejects_containment_before_any_device(hg, tmp_path):
    out = tmp_path / "out.tsv"
    r = run(hg, "cluster", "-p", str(tmp_path / "missing.sketch"), "-o", str(out), "--ani_metric", "containment")
    assert r.returncode != 0
    assert "--ani_metric containment is not supported by cluster" in r.stderr
    assert not out.exists()


@pytest.mark.parametrize("metric", [cr.CONTAINMENT, cr.MAX_CONTAINMENT])
def test_formula_equals_mash_on_equal_norms(orc, metric):
    """with nr = nq = n, 2J / (1 + J) = dot / n: the containment forms give the Mash-style value up to rounding"""
    rng = np.random.default_rng(11 + metric)
    N = 100_000
    n = rng.integers(1_000, 1 << 26, N).astype(np.int32)
    dot = (n * rng.uniform(0.02, 1.0, N)).astype(np.int32)
    for k in (15, 21, 32):
        want = orc.ani_from_dots(dot, n, n, k)
        got = cr.ani_ref(orc, dot, n, n, k, metric)
        ok = want > 0  # (both clamp to 0 together far below any threshold)
        ulp = np.abs(got[ok].view(np.int32).astype(np.int64) - want[ok].view(np.int32).astype(np.int64))
        assert ulp.max() <= 4, (k, int(ulp.max()))
        assert ((got == 0) == (want == 0)).mean() > 0.999


def test_formula_edge_cases(orc):
    k = 21
    dot = np.array([0, -5, 0, 7, 200, 100], np.int32)
    nr = np.array([100, 100, 0, 0, 100, 100], np.int32)
    nq = np.array([100, 100, 0, 0, 100, 50], np.int32)
    for m in (cr.CONTAINMENT, cr.MAX_CONTAINMENT):
        got = cr.ani_ref(orc, dot, nr, nq, k, m)
        assert list(got[:5]) == [0.0, 0.0, 0.0, 100.0, 100.0]  # dot <= 0, 0 / 0, x / 0, dot > den
    assert cr.ani_ref(orc, dot, nr, nq, k, cr.CONTAINMENT)[5] == 100.0  # 100 / nq = 2
    assert cr.ani_ref(orc, dot, nr, nq, k, cr.MAX_CONTAINMENT)[5] == 100.0
