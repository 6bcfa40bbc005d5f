"""The row blocks of the symmetric comparison under the four clustering schemes (hg_cluster_dev, hg_cluster_greedy_dev,
hg_cluster_setcover_dev, hg_cluster_tree_dev and their host forms) at the sizes where the block walk has its edges: one
sketch, two, an empty block in the middle, a last block of a single row, a first block that overflows the hit list and
runs again, a list that grows while it keeps the earlier blocks' hits.  Every result EQUALS, bit for bit, the scheme's
model (tests/cluster_*_ref.py, the union-find of test_gpu_cluster.py) on the hits of a plain hg_dist_dev call over the
same rows; the rounds counters are pinned to what the schemes ran when this file was written."""
import os
import sys

import numpy as np
import pytest

import cluster_greedy_ref as gr
import cluster_setcover_ref as sr
import cluster_tree_ref as tr
from test_gpu_cluster import model as components

pytestmark = pytest.mark.gpu

TH = 95.0
# rows of bench.clustered_hvs(200, 0): 0, 1, 2 lie in one group of 100 (pairs at or above TH), 100 in the next (below TH)
ORDERS = [(0,), (0, 1), (0, 100), (0, 100, 1), (0, 1, 2, 100), (1, 100, 0, 2)]
HOOKS = [None, {"pair_limit": "1", "cluster_hit_cap": "1"}]  # the second: one row per block, a list of one record at first
# rounds of the _dev forms, (no hooks, one row per block): read off a run of this file's `rounds_of` when it was written
ROUNDS = {
    "greedy": {(0,): (1, 1), (0, 1): (2, 2), (0, 100): (1, 2), (0, 100, 1): (2, 3), (0, 1, 2, 100): (2, 4), (1, 100, 0, 2): (2, 4)},
    "setcover": {order: (1, 1) for order in ORDERS},
    "tree": {(0,): (0, 0), (0, 1): (2, 2), (0, 100): (0, 0), (0, 100, 1): (2, 2), (0, 1, 2, 100): (2, 4), (1, 100, 0, 2): (2, 4)},
}


def build_cases():
    """the four sketches the orders draw from, and per order the hits of hg_dist_dev with the models' answers (computed once,
    on a ctx of its own)"""
    import torch
    import hypergen_amd as hg
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import bench
    dev = torch.device("cuda:0")
    hv_all = bench.clustered_hvs(200, 0, dev)
    cases = {}
    with hg.Context(0) as c:
        for order in ORDERS:
            n = len(order)
            hv = hv_all[list(order)].contiguous()
            n2 = (hv.int() ** 2).sum(1).int()
            full = torch.empty(n * n, dtype=torch.float32, device=dev)
            out = torch.empty(3 * n * n, dtype=torch.int32, device=dev)
            torch.cuda.synchronize()
            c.dist_full_dev(hv.data_ptr(), n2.data_ptr(), n, hv.data_ptr(), n2.data_ptr(), n, hv.shape[1], 21, full.data_ptr())
            found, st = c.dist_dev(hv.data_ptr(), n2.data_ptr(), n, hv.data_ptr(), n2.data_ptr(), n, hv.shape[1], 21, True, TH,
                                   out.data_ptr(), n * n)
            c.sync()
            assert st == 0
            m = full.cpu().numpy().reshape(n, n)
            for i in range(n):
                for j in range(n):
                    if i != j:  # one group of 100 passes, different groups do not
                        assert (m[i, j] >= np.float32(TH)) == (order[i] // 100 == order[j] // 100), (order, i, j, m[i, j])
            h = out[:3 * found].cpu().numpy().view(np.uint8).view(hg.ANI_HIT_DTYPE)
            a, b, ani = h["ref_idx"], h["qry_idx"], h["ani"]
            assert found == sum(order[i] // 100 == order[j] // 100 for i in range(n) for j in range(i + 1, n))
            cases[order] = {
                "hv": hv, "n2": n2, "hv_host": hv.cpu().numpy(), "n2_host": n2.cpu().numpy(),
                "single": components(n, a, b),
                "greedy": gr.greedy_model(n, a, b, ani, TH),
                "setcover": sr.setcover_model(n, a, b, ani, TH),
                "tree": tr.tree_model(n, a, b, ani, TH),
            }
    return cases


@pytest.fixture(scope="module")
def rows():
    return build_cases()


@pytest.fixture
def ctx():
    """a fresh ctx per test: no earlier call's hit list shows through"""
    import hypergen_amd as hg
    with hg.Context(0) as c:
        yield c


def set_hooks(c, hooks):
    for k in ("pair_limit", "cluster_hit_cap"):
        c.set_debug(k, (hooks or {}).get(k, "0"))


def u32(t):
    return t.cpu().numpy().view(np.uint32)


def run_dev(c, scheme, case):
    """the _dev form -> the scheme's result tuple as numpy (ani and tree as stored), and the rounds counter behind it"""
    import torch
    import hypergen_amd as hg
    hv, n2 = case["hv"], case["n2"]
    n, D, dev = hv.shape[0], hv.shape[1], hv.device
    rep = torch.empty(n, dtype=torch.int32, device=dev)
    cl = torch.empty(n, dtype=torch.int32, device=dev)
    ani = torch.empty(n, dtype=torch.float32, device=dev)
    tree = torch.empty(3 * max(n - 1, 1), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()  # (the ctx runs on its own stream)
    if scheme == "single":
        nc = c.cluster_dev(hv.data_ptr(), n2.data_ptr(), n, D, rep.data_ptr(), cl.data_ptr(), 21, TH)
        return (u32(rep), u32(cl), nc), None
    if scheme == "greedy":
        nc = c.cluster_greedy_dev(hv.data_ptr(), n2.data_ptr(), n, D, rep.data_ptr(), cl.data_ptr(), ani.data_ptr(), 21, TH)
        return (u32(rep), u32(cl), ani.cpu().numpy(), nc), c.cluster_greedy_rounds()
    if scheme == "setcover":
        nc = c.cluster_setcover_dev(hv.data_ptr(), n2.data_ptr(), n, D, rep.data_ptr(), cl.data_ptr(), ani.data_ptr(), 21, TH)
        return (u32(rep), u32(cl), ani.cpu().numpy(), nc), c.cluster_setcover_rounds()
    ne, nc = c.cluster_tree_dev(hv.data_ptr(), n2.data_ptr(), n, D, tree.data_ptr(), n - 1, rep.data_ptr(), cl.data_ptr(), 21, TH)
    t = tree[:3 * ne].cpu().numpy().view(np.uint8).view(hg.ANI_HIT_DTYPE)
    return (t, u32(rep), u32(cl), nc), c.cluster_tree_rounds()


def run_host(c, scheme, case):
    hv, n2 = case["hv_host"], case["n2_host"]
    return {"single": c.cluster, "greedy": c.cluster_greedy, "setcover": c.cluster_setcover, "tree": c.cluster_tree}[scheme](hv, n2, 21, TH)


def assert_same(scheme, got, want):
    """rep, cluster, ani (as uint32), tree edges and counts, bit for bit"""
    assert len(got) == len(want)
    assert got[-1] == want[-1], (scheme, "cluster count")
    for g, w in zip(got[:-1], want[:-1]):
        g, w = np.ascontiguousarray(g), np.ascontiguousarray(w)
        assert g.size == w.size, scheme
        assert g.view(np.uint8).tobytes() == w.view(np.uint8).tobytes(), (scheme, g, w)


SCHEMES = ["single", "greedy", "setcover", "tree"]


@pytest.mark.parametrize("hooks", HOOKS, ids=["whole", "row_blocks"])
@pytest.mark.parametrize("order", ORDERS, ids=lambda o: "-".join(map(str, o)))
def test_every_scheme_equals_its_model(rows, ctx, order, hooks):
    case = rows[order]
    set_hooks(ctx, hooks)
    for scheme in SCHEMES:
        got, _ = run_dev(ctx, scheme, case)
        assert_same(scheme, got, case[scheme])
        if scheme == "tree":
            assert got[0].size == len(order) - got[3]
        assert_same(scheme, run_host(ctx, scheme, case), case[scheme])


def rounds_of(ctx, case):
    """{scheme: (rounds without hooks, rounds with one row per block)} of the _dev forms"""
    out = {}
    for scheme in SCHEMES[1:]:
        per = []
        for hooks in HOOKS:
            set_hooks(ctx, hooks)
            per.append(run_dev(ctx, scheme, case)[1])
        out[scheme] = tuple(per)
    return out


@pytest.mark.parametrize("order", ORDERS, ids=lambda o: "-".join(map(str, o)))
def test_rounds_are_what_they_were(rows, ctx, order):
    got = rounds_of(ctx, rows[order])
    print("rounds", order, got)
    for scheme, pair in got.items():
        assert pair == ROUNDS[scheme][order], (scheme, order, pair)


def test_no_sketches(ctx):
    """n = 0: no clusters, no edges, HG_OK (the call raises otherwise)"""
    import torch
    dev = torch.device("cuda:0")
    hv = torch.zeros(1024, dtype=torch.int16, device=dev)
    w = torch.zeros(16, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    p = w.data_ptr()
    for hooks in HOOKS:
        set_hooks(ctx, hooks)
        assert ctx.cluster_dev(hv.data_ptr(), p, 0, 1024, p, p, 21, TH) == 0
        assert ctx.cluster_greedy_dev(hv.data_ptr(), p, 0, 1024, p, p, p, 21, TH) == 0
        assert ctx.cluster_setcover_dev(hv.data_ptr(), p, 0, 1024, p, p, p, 21, TH) == 0
        assert ctx.cluster_tree_dev(hv.data_ptr(), p, 0, 1024, p, 0, p, p, 21, TH) == (0, 0)
