"""`hyper-gen cluster` and the hg_cluster* entry points, the parts that need no GPU: the command line's surface (help,
required arguments, what it rejects before a device is opened) and the C ABI's declarations and exports."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("hg_cluster_init_dev", "hg_cluster_add_hits_dev", "hg_cluster_finish_dev", "hg_cluster_dev", "hg_cluster")


@pytest.fixture(scope="module")
def hg():
    import hypergen_amd
    hypergen_amd.lib()
    return hypergen_amd


def run(hg, *args):
    return subprocess.run([hg.CLI_PATH] + list(args), capture_output=True, text=True, timeout=60)


def test_help_lists_cluster(hg):
    r = run(hg, "--help")
    assert r.returncode == 0
    assert "hyper-gen cluster -p" in r.stdout
    assert "95.0" in r.stdout  # cluster's own default threshold
    assert "<sketch|dist|search|cluster>" in run(hg).stderr


def test_cluster_requires_path_and_out(hg, tmp_path):
    for args in ((), ("-p", str(tmp_path / "x.sketch")), ("-o", str(tmp_path / "out.tsv"))):
        r = run(hg, "cluster", *args)
        assert r.returncode != 0
        assert "required arguments were not provided: --path --out" in r.stderr


def test_cluster_rejects_shards_before_any_device(hg, tmp_path):
    # the file does not exist and no device is needed: the option is refused first
    r = run(hg, "cluster", "-p", str(tmp_path / "missing.sketch"), "-o", str(tmp_path / "out.tsv"), "--shards", "2")
    assert r.returncode != 0
    assert "--shards is not supported by cluster" in r.stderr
    assert not (tmp_path / "out.tsv").exists()


def test_cluster_symbols_declared_and_exported(hg):
    hdr = open(os.path.join(ROOT, "include", "hypergen.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    nm = subprocess.run(["nm", "-D", "--defined-only", hg.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r"\bT (hg_\w+)", nm))
    for name in NAMES:
        assert re.search(r"\bhg_status %s\(" % name, hdr), name
        assert name in exported, name
        assert name in hg.EXPORTS, name
    hdr_full = open(os.path.join(ROOT, "include", "hypergen.h")).read()
    assert '"cluster_hit_cap"' in hdr_full
