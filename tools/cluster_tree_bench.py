"""hg_cluster_tree_dev against the routes it replaces (bench.clustered_hvs: clusters of 100 members, ~96-97 % ANI inside a
cluster): per size, at a floor of 95 and at a floor of 90, the wall ms of
  tree          hg_cluster_tree_dev at the floor (tree + rep / cluster);
  tree_levels   the same plus two more levels cut from the tree (hg_cluster_init_dev + hg_cluster_add_hits_dev +
                hg_cluster_finish_dev per level): three levels from one comparison;
  single        hg_cluster_dev at the floor;
  per_level     hg_cluster_dev once per level for the three levels -- the route the feature replaces.
The legs alternate in one process, --rounds times; each leg of a round is the median wall ms of --steps calls (every call
returns with its results final).  Prints one JSON line and writes it to profiles/cluster_tree_bench.json: per size and
floor the hits the comparison enumerates, the tree's edges, the clusters per level, the rounds of the tree call
(hg_ctx_cluster_tree_rounds) and per leg the median of the rounds with min and max; and -- from a second run of this
script under `rocprofv3 --kernel-trace --stats` -- the tree kernels' own device ms per hg_cluster_tree_dev call.  No ratio is
a pass condition.

    python tools/cluster_tree_bench.py [--n 10000 100000] [--rounds 3 --steps 3 --warmup 1] [--no-prof] [--no-write]
"""
import argparse
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LEVELS = {95.0: (95.0, 97.0, 99.0), 90.0: (90.0, 95.0, 99.0)}


def median_ms(fn, steps):
    ts = []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts.sort()
    return ts[len(ts) // 2]


def summary(v):
    s = sorted(v)
    return {"median_ms": round(s[len(s) // 2], 3), "min_ms": round(s[0], 3), "max_ms": round(s[-1], 3)}


def measure_one(c, hg, torch, bench, n, a):
    dev = torch.device("cuda:0")
    hv = bench.clustered_hvs(n, 0, dev)
    n2 = (hv.int() ** 2).sum(1).int()
    D = hv.shape[1]
    tree = torch.empty(3 * max(n - 1, 1), dtype=torch.int32, device=dev)
    one = torch.empty(3, dtype=torch.int32, device=dev)
    rep = torch.empty(n, dtype=torch.int32, device=dev)
    cl = torch.empty(n, dtype=torch.int32, device=dev)
    rep2 = torch.empty(n, dtype=torch.int32, device=dev)
    cl2 = torch.empty(n, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    rows = []
    for floor, levels in LEVELS.items():
        res = {}

        def tree_leg():
            res["tree_edges"], res["clusters_floor"] = c.cluster_tree_dev(hv.data_ptr(), n2.data_ptr(), n, D, tree.data_ptr(), n - 1,
                                                                          rep.data_ptr(), cl.data_ptr(), 21, floor)
            res["tree_rounds"] = c.cluster_tree_rounds()

        def tree_levels_leg():
            tree_leg()
            counts = [res["clusters_floor"]]
            for t in levels[1:]:
                c.cluster_init_dev(rep2.data_ptr(), n)
                c.cluster_add_hits_dev(rep2.data_ptr(), n, tree.data_ptr(), res["tree_edges"], t)
                counts.append(c.cluster_finish_dev(rep2.data_ptr(), n, cl2.data_ptr()))
            res["clusters_from_tree"] = counts

        def single_leg():
            res["single_clusters_floor"] = c.cluster_dev(hv.data_ptr(), n2.data_ptr(), n, D, rep2.data_ptr(), cl2.data_ptr(), 21, floor)

        def per_level_leg():
            res["clusters_per_level"] = [c.cluster_dev(hv.data_ptr(), n2.data_ptr(), n, D, rep2.data_ptr(), cl2.data_ptr(), 21, t)
                                         for t in levels]

        legs = {"tree": tree_leg, "tree_levels": tree_levels_leg, "single": single_leg, "per_level": per_level_leg}
        if a.only:
            legs = {a.only: legs[a.only]}
        else:  # the hits the comparison enumerates at the floor (counted, not stored)
            res["hits"], _ = c.dist_dev(hv.data_ptr(), n2.data_ptr(), n, hv.data_ptr(), n2.data_ptr(), n, D, 21, True, floor, one.data_ptr(), 1)
        for fn in legs.values():
            for _ in range(a.warmup):
                fn()
        per = {k: [] for k in legs}
        for _ in range(a.rounds):
            for k, fn in legs.items():
                per[k].append(median_ms(fn, a.steps))
        row = {"n": n, "floor": floor, "levels": list(levels), **res}
        for k in legs:
            row[k] = summary(per[k])
        if not a.only:
            assert res["clusters_from_tree"] == res["clusters_per_level"], "the cuts of the tree are the per-level clusters"
            row["tree_over_single"] = round(row["tree"]["median_ms"] / row["single"]["median_ms"], 3)
            row["tree_levels_over_per_level"] = round(row["tree_levels"]["median_ms"] / row["per_level"]["median_ms"], 3)
        rows.append(row)
    return rows


def measure(a):
    import torch
    import hypergen_amd as hg
    import bench
    rows = []
    with hg.Context(0) as c:
        for n in a.n:
            rows += measure_one(c, hg, torch, bench, n, a)
    return rows


def kernel_ms(a):
    """per hg_cluster_tree_dev call: device ms of the tree kernels, the radix passes of the final order and the finishing
    kernels shared with hg_cluster_dev (rocprofv3 --kernel-trace --stats of a run of the tree leg alone, all sizes and floors
    together)"""
    d = tempfile.mkdtemp(prefix="cluster_tree_prof_")
    try:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable,
               os.path.abspath(__file__), "--n"] + [str(n) for n in a.n] + ["--rounds", str(a.rounds), "--steps", str(a.steps),
                                                                            "--warmup", str(a.warmup), "--no-prof", "--no-write",
                                                                            "--only", "tree"]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=1100)
        if r.returncode != 0:
            return None, "rocprofv3 exit %d" % r.returncode
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            return None, "no kernel_stats.csv"
        calls = len(a.n) * len(LEVELS) * (a.warmup + a.rounds * a.steps)
        per = {}
        with open(files[0]) as f:
            for row in csv.DictReader(f):
                name = row["Name"]
                if ("tree_" in name or "cluster_" in name or "radix_" in name) and "_kernel" in name:
                    short = name.split("::")[-1].split("(")[0].split("<")[0]
                    per[short] = per.get(short, 0.0) + float(row["TotalDurationNs"]) / 1e6 / calls
        return {k: round(v, 5) for k, v in sorted(per.items())}, None
    finally:
        shutil.rmtree(d, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[10_000, 100_000])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--only", choices=["tree", "tree_levels", "single", "per_level"], default=None)
    ap.add_argument("--no-prof", action="store_true")
    ap.add_argument("--no-write", action="store_true")
    a = ap.parse_args()
    out = {"bench": "cluster_tree", "rounds": a.rounds, "steps": a.steps, "cases": measure(a)}
    if not a.no_prof:
        per, err = kernel_ms(a)
        out["kernels_ms_per_tree_call"] = per  # (averaged over every size and floor of the profiled run)
        if err:
            out["kernels_error"] = err
    line = json.dumps(out)
    print(line)
    if not a.no_write and not a.only:
        with open(os.path.join(ROOT, "profiles", "cluster_tree_bench.json"), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
