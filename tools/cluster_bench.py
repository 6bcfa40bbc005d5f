"""hg_cluster_dev against the thresholded symmetric hg_dist_dev of the same matrix (bench.clustered_hvs: clusters of 100
members, ~96-97 % ANI inside a cluster).  Prints one JSON line: n, ani_th, the hit count, the cluster count, the median
wall ms of both calls (each returns with its results final) and -- from a second run of this script under
`rocprofv3 --kernel-trace --stats` -- the clustering kernels' own device ms per hg_cluster_dev call.

    python tools/cluster_bench.py --n 10000 --ani_th 95 [--steps 20 --warmup 3] [--no-prof]
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


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts.sort()
    return ts[len(ts) // 2]


def measure(a):
    import torch
    import numpy as np  # noqa: F401
    import hypergen_amd as hg
    import bench
    dev = torch.device("cuda:0")
    hv = bench.clustered_hvs(a.n, 0, dev)
    n2 = (hv.int() ** 2).sum(1).int()
    D = hv.shape[1]
    torch.cuda.synchronize()
    with hg.Context(0) as c:
        pairs = a.n * (a.n - 1) // 2
        cap = min(pairs, 16_000_000)
        out = torch.empty(3 * max(cap, 1), dtype=torch.int32, device=dev)
        rep = torch.empty(a.n, dtype=torch.int32, device=dev)
        cl = torch.empty(a.n, dtype=torch.int32, device=dev)
        res = {}

        def dist():
            res["hits"], st = c.dist_dev(hv.data_ptr(), n2.data_ptr(), a.n, hv.data_ptr(), n2.data_ptr(), a.n, D, 21, True, a.ani_th,
                                         out.data_ptr(), cap)
            assert st == 0, "hit buffer too small"

        def clu():
            res["n_clusters"] = c.cluster_dev(hv.data_ptr(), n2.data_ptr(), a.n, D, rep.data_ptr(), cl.data_ptr(), 21, a.ani_th)

        dist_ms = timed(dist, a.steps, a.warmup)
        clu_ms = timed(clu, a.steps, a.warmup)
    return {"n": a.n, "ani_th": a.ani_th, "hits": res["hits"], "n_clusters": res["n_clusters"], "dist_ms": round(dist_ms, 4),
            "cluster_ms": round(clu_ms, 4), "ratio": round(clu_ms / dist_ms, 3), "calls": a.steps + a.warmup}


def kernel_ms(a, calls):
    """per hg_cluster_dev call: device ms of the clustering kernels (rocprofv3 --kernel-trace --stats of a --no-prof run)"""
    d = tempfile.mkdtemp(prefix="cluster_prof_")
    try:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable,
               os.path.abspath(__file__), "--n", str(a.n), "--ani_th", str(a.ani_th), "--steps", str(a.steps),
               "--warmup", str(a.warmup), "--no-prof"]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            return None, "rocprofv3 exit %d" % r.returncode
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            return None, "no kernel_stats.csv"
        per = {}
        with open(files[0]) as f:
            for row in csv.DictReader(f):
                name = row["Name"]
                if "cluster_" in name and "_kernel" in name:
                    short = name.split("::")[-1].split("(")[0]
                    per[short] = per.get(short, 0.0) + float(row["TotalDurationNs"]) / 1e6 / calls
        return {k: round(v, 5) for k, v in sorted(per.items())}, None
    finally:
        shutil.rmtree(d, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000)
    ap.add_argument("--ani_th", type=float, default=95.0)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-prof", action="store_true")
    a = ap.parse_args()
    out = measure(a)
    if not a.no_prof:
        # (the kernel times of every hg_cluster_dev call of the profiled run: warm-up and timed ones)
        per, err = kernel_ms(a, out["calls"])
        out["kernels_ms"] = per
        out["kernels_total_ms"] = round(sum(per.values()), 5) if per else None
        if err:
            out["kernels_error"] = err
    print(json.dumps(out))


if __name__ == "__main__":
    main()
