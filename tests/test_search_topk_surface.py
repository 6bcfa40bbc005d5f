"""CPU-side checks of the bounded-memory search (hg_search_topk*): the symbols are declared, listed and exported, the CLI
knows --search_path, and the numpy model the GPU tests compare with (tests/search_topk_ref.py) equals a plain loop."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import search_topk_ref as ref

SYMBOLS = ("hg_search_topk_dev", "hg_search_topk_block_dev", "hg_search_topk", "hg_search_topk_merge", "hg_search_topk_multi_dev")


@pytest.fixture(scope="module")
def hg():
    import hypergen_amd
    hypergen_amd.lib()
    return hypergen_amd


def header():
    return open(os.path.join(ROOT, "include", "hypergen.h")).read()


def test_search_topk_symbols_are_declared_listed_and_exported(hg):
    decl = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    nm = subprocess.run(["nm", "-D", "--defined-only", hg.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\b(hg_[a-z0-9_]+)$", nm, flags=re.M))
    for s in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, decl), "%s is not declared in include/hypergen.h" % s
        assert s in hg.EXPORTS, "%s is missing from EXPORTS" % s
        assert s in exported, "%s is not exported by the library" % s
        assert hasattr(hg.lib(), s)


def test_search_topk_max_is_64_and_the_block_budget_is_documented(hg):
    hdr = header()
    assert re.search(r"#define\s+HG_SEARCH_TOPK_MAX\s+64u\b", hdr)
    assert re.search(r"#define\s+HG_SEARCH_BLOCK_BYTES\s+\(\(size_t\)256 << 20\)", hdr)
    assert '"search_block_rows"' in hdr
    assert hg.SEARCH_TOPK_MAX == 64


def test_search_topk_kernels_exist_and_stay_out_of_the_census_families(hg):
    nm = subprocess.run(["nm", "-C", hg.LIB_PATH], capture_output=True, text=True, check=True).stdout
    kernels = set(re.findall(r"::(search_topk_[a-z0-9_]+)\(", nm))
    assert {"search_topk_select_kernel", "search_topk_merge_kernel", "search_topk_emit_kernel"} <= kernels
    census = re.compile(r"dist_.*kernel|kmer_sample_|sort_unique|bucket_.*_kernel|encode.*_kernel|sketch_finish_kernel|min_count_")
    for k in kernels:
        assert not census.match(k), k


def test_cli_help_names_search_path_and_bad_uses_are_rejected(hg):
    r = subprocess.run([hg.CLI_PATH, "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "--search_path auto|hits|topk" in r.stdout
    bad = (["search", "--search_path", "fast"],           # not a value
           ["search", "--search_path", "topk", "-n", "65"],  # the fused path stops at HG_SEARCH_TOPK_MAX
           ["search", "-n", "65", "--search_path", "topk"],  # ... in either order
           ["dist", "--search_path", "topk"],             # search only
           ["sketch", "--search_path", "auto"],
           ["cluster", "--search_path", "hits"])
    for args in bad:
        r = subprocess.run([hg.CLI_PATH] + args, capture_output=True, text=True)
        assert r.returncode == 2 and "search_path" in r.stderr, (args, r.returncode, r.stderr)
    # accepted values parse (without -r / -q / -o `search` stays the no-op it was)
    for v in ("auto", "hits", "topk"):
        assert subprocess.run([hg.CLI_PATH, "search", "--search_path", v], capture_output=True).returncode == 0
    assert subprocess.run([hg.CLI_PATH, "search", "--search_path=topk", "-n", "64"], capture_output=True).returncode == 0


def test_merge_is_host_only_and_follows_the_order(hg):
    """hg_search_topk_merge needs no device: two shards' lists with ties across them"""
    k = 3
    a = np.zeros((2, k), ref.HIT_DTYPE)
    b = np.zeros((2, k), ref.HIT_DTYPE)
    for x in (a, b):
        x["ref_idx"] = x["qry_idx"] = ref.EMPTY
    a[0, :2] = [(4, 0, 99.0), (1, 0, 97.5)]
    b[0, :3] = [(7, 0, 99.0), (9, 0, 97.5), (8, 0, 90.0)]
    b[1, :1] = [(12, 1, 0.0)]
    out, cnt = hg.search_topk_merge([a, b], [np.array([2, 0], np.uint32), np.array([3, 1], np.uint32)], k)
    assert cnt.tolist() == [3, 1]
    assert out[0].tolist() == [(4, 0, 99.0), (7, 0, 99.0), (1, 0, 97.5)]
    assert out[1].tolist() == [(12, 1, 0.0), (ref.EMPTY, ref.EMPTY, 0.0), (ref.EMPTY, ref.EMPTY, 0.0)]
    assert hg.lib().hg_search_topk_merge(None, None, 0, 2, 65, None, None) == hg.ERR_UNSUPPORTED
    assert hg.lib().hg_search_topk_merge(None, None, 0, 2, 0, None, None) == hg.OK
    assert hg.lib().hg_search_topk_merge(None, None, 1, 2, 1, None, None) == hg.ERR_INVALID


@pytest.mark.parametrize("R,Q", [(1, 1), (5, 1), (7, 3), (40, 9), (130, 5)])
def test_model_equals_a_plain_loop_on_matrices_full_of_ties(R, Q):
    rng = np.random.default_rng(R * 131 + Q)
    # few distinct values, among them 0 and 100: ties everywhere, and thresholds that hit values exactly
    vals = np.array([0.0, 0.0, 84.99999, 85.0, 85.00001, 99.5, 100.0], np.float32)
    ani = vals[rng.integers(0, vals.size, (R, Q))]
    top = ref.topk_sorted(ani, 64, chunk=3)  # ordered once, cut by every (threshold, k): the form the GPU tests sweep with
    for k in (1, 2, 5, 64):
        for th in (0.0, 85.0, 99.5, 100.0, 101.0):
            got, gc = ref.topk_model(ani, th, k, chunk=4)
            want, wc = ref.topk_loop(ani, th, k)
            swept, sc = ref.topk_from_sorted(top, th, k)
            assert np.array_equal(swept, want) and np.array_equal(sc, wc), (R, Q, k, th)
            assert np.array_equal(gc, wc), (R, Q, k, th)
            assert np.array_equal(got, want), (R, Q, k, th)
            assert (gc <= k).all() and all((got["ref_idx"][q, gc[q]:] == ref.EMPTY).all() for q in range(Q))


def test_model_offsets_and_empty_inputs():
    ani = np.array([[90.0, 10.0], [90.0, 95.0]], np.float32)
    h, c = ref.topk_model(ani, 50.0, 2, ref_off=100, qry_off=7)
    assert c.tolist() == [2, 1]
    assert h[0].tolist() == [(100, 7, 90.0), (101, 7, 90.0)] and h[1, 0].tolist() == (101, 8, 95.0)
    h, c = ref.topk_model(np.zeros((0, 3), np.float32), 0.0, 2)
    assert c.tolist() == [0, 0, 0] and (h["ref_idx"] == ref.EMPTY).all()
