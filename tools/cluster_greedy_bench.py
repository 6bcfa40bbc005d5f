"""hg_cluster_greedy_dev against hg_cluster_dev and against the thresholded symmetric hg_dist_dev of the same matrix
(bench.clustered_hvs: clusters of 100 members, ~96-97 % ANI inside a cluster): what the greedy resolution costs on top of
the same GEMM.  Two thresholds per size: 95 (every group a complete clique) and the median within-cluster ANI (read from
hg_dist_full_dev of rows 0..299: partial cliques).  The three legs alternate in one process, --rounds times; each leg of
a round is the median wall ms of --steps calls (every call returns with its results final).  Prints one JSON line: per
size and threshold the hit count, the clusters of both linkages, the rounds of the greedy call
(hg_ctx_cluster_greedy_rounds) and per leg the median of the rounds with min and max; and -- from a second run of this
script under `rocprofv3 --kernel-trace --stats` -- the greedy kernels' own device ms per hg_cluster_greedy_dev call.

    python tools/cluster_greedy_bench.py [--n 10000 100000] [--rounds 3 --steps 3 --warmup 1] [--no-prof]
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
    import numpy as np
    dev = torch.device("cuda:0")
    hv = bench.clustered_hvs(n, 0, dev)
    n2 = (hv.int() ** 2).sum(1).int()
    D = hv.shape[1]
    full = torch.empty(300 * 300, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    c.dist_full_dev(hv.data_ptr(), n2.data_ptr(), 300, hv.data_ptr(), n2.data_ptr(), 300, D, 21, full.data_ptr())
    c.sync()
    m = full.cpu().numpy().reshape(300, 300)
    i, j = np.triu_indices(300, 1)
    band = float(np.median(m[i, j][i // 100 == j // 100]))
    cap = min(n * (n - 1) // 2, 16_000_000)
    out = torch.empty(3 * max(cap, 1), dtype=torch.int32, device=dev)
    rep = torch.empty(n, dtype=torch.int32, device=dev)
    cl = torch.empty(n, dtype=torch.int32, device=dev)
    ani = torch.empty(n, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    rows = []
    for th in (95.0, band):
        res = {}

        def dist():
            res["hits"], st = c.dist_dev(hv.data_ptr(), n2.data_ptr(), n, hv.data_ptr(), n2.data_ptr(), n, D, 21, True, th,
                                         out.data_ptr(), cap)
            assert st == 0, "hit buffer too small"

        def single():
            res["single_clusters"] = c.cluster_dev(hv.data_ptr(), n2.data_ptr(), n, D, rep.data_ptr(), cl.data_ptr(), 21, th)

        def greedy():
            res["greedy_clusters"] = c.cluster_greedy_dev(hv.data_ptr(), n2.data_ptr(), n, D, rep.data_ptr(), cl.data_ptr(),
                                                          ani.data_ptr(), 21, th)
            res["greedy_rounds"] = c.cluster_greedy_rounds()

        legs = {"dist": dist, "single": single, "greedy": greedy}
        if a.only:
            legs = {a.only: legs[a.only]}
        for fn in legs.values():
            for _ in range(a.warmup):
                fn()
        per = {k: [] for k in legs}
        for _ in range(a.rounds):
            for k, fn in legs.items():
                per[k].append(median_ms(fn, a.steps))
        row = {"n": n, "ani_th": round(th, 4), **res}
        for k in legs:
            row[k] = summary(per[k])
        if not a.only:
            row["greedy_over_single"] = round(row["greedy"]["median_ms"] / row["single"]["median_ms"], 3)
            row["greedy_over_dist"] = round(row["greedy"]["median_ms"] / row["dist"]["median_ms"], 3)
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
    """per hg_cluster_greedy_dev call: device ms of the greedy kernels and of the finishing kernels they share with
    hg_cluster_dev (rocprofv3 --kernel-trace --stats of a run of the greedy leg alone, all sizes and thresholds together)"""
    d = tempfile.mkdtemp(prefix="cluster_greedy_prof_")
    try:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable,
               os.path.abspath(__file__), "--n"] + [str(n) for n in a.n] + ["--rounds", str(a.rounds), "--steps", str(a.steps),
                                                                            "--warmup", str(a.warmup), "--no-prof", "--only", "greedy"]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=1100)
        if r.returncode != 0:
            return None, "rocprofv3 exit %d" % r.returncode
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            return None, "no kernel_stats.csv"
        calls = len(a.n) * 2 * (a.warmup + a.rounds * a.steps)
        per = {}
        with open(files[0]) as f:
            for row in csv.DictReader(f):
                name = row["Name"]
                if ("greedy_" in name or "cluster_" in name) and "_kernel" in name:
                    short = name.split("::")[-1].split("(")[0]
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
    ap.add_argument("--only", choices=["dist", "single", "greedy"], default=None)
    ap.add_argument("--no-prof", action="store_true")
    a = ap.parse_args()
    out = {"bench": "cluster_greedy", "rounds": a.rounds, "steps": a.steps, "cases": measure(a)}
    if not a.no_prof:
        per, err = kernel_ms(a)
        out["kernels_ms_per_greedy_call"] = per  # (averaged over every size and threshold of the profiled run)
        if err:
            out["kernels_error"] = err
    print(json.dumps(out))


if __name__ == "__main__":
    main()
