"""hg_cluster_average_dev against hg_cluster_dev and against hg_dist_full_dev of the same sketches (bench.clustered_hvs:
clusters of 100 members, ~96-97 % ANI inside a cluster): what average linkage -- the dense n x n matrix of u64 sums, filled
from blocks of the ANI matrix, and four launches per round over it -- costs on top of the comparison it needs anyway (the
full matrix: the pairs below the threshold enter the averages) and against single linkage, which gets by with the
thresholded one.  Two thresholds per size: 95 and the median within-cluster ANI (read from hg_dist_full_dev of rows
0..299).  The three legs alternate in one process, --rounds times; each leg of a round is the median wall ms of --steps
calls (every call returns with its results final).  Prints one JSON line and writes it to
profiles/cluster_average_bench.json: per size and threshold the clusters of average and of single linkage, the rounds of
the average-linkage call (hg_ctx_cluster_average_rounds), the matrix held and per leg the median of the rounds with min and
max.  No ratio is a pass condition.

    python tools/cluster_average_bench.py [--n 10000 30000] [--rounds 3 --steps 3 --warmup 1] [--no-write]
"""
import argparse
import json
import os
import sys
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


def measure_one(c, torch, bench, n, a):
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
    full = torch.empty(n * n, dtype=torch.float32, device=dev)
    rep = torch.empty(n, dtype=torch.int32, device=dev)
    cl = torch.empty(n, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    rows = []
    for th in (95.0, band):
        res = {}

        def dist_full():
            c.dist_full_dev(hv.data_ptr(), n2.data_ptr(), n, hv.data_ptr(), n2.data_ptr(), n, D, 21, full.data_ptr())
            c.sync()

        def single():
            res["single_clusters"] = c.cluster_dev(hv.data_ptr(), n2.data_ptr(), n, D, rep.data_ptr(), cl.data_ptr(), 21, th)

        def average():
            res["average_clusters"] = c.cluster_average_dev(hv.data_ptr(), n2.data_ptr(), n, D, rep.data_ptr(), cl.data_ptr(),
                                                            None, None, None, 21, th)
            res["average_rounds"] = c.cluster_average_rounds()

        legs = {"dist_full": dist_full, "single": single, "average": average}
        for fn in legs.values():
            for _ in range(a.warmup):
                fn()
        per = {k: [] for k in legs}
        for _ in range(a.rounds):
            for k, fn in legs.items():
                per[k].append(median_ms(fn, a.steps))
        row = {"n": n, "ani_th": round(th, 4), **res, "matrix_mb": round(n * ((n + 1) // 2 * 2) * 8 / 1e6, 1)}
        for k in legs:
            row[k] = summary(per[k])
        rows.append(row)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[10_000, 30_000])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--no-write", action="store_true")
    a = ap.parse_args()
    import torch
    import hypergen_amd as hg
    import bench
    rows = []
    with hg.Context(0) as c:
        for n in a.n:
            rows += measure_one(c, torch, bench, n, a)
    out = {"bench": "cluster_average", "status": "measured", "rounds": a.rounds,
           "steps": a.steps, "launches_per_round": 4, "cases": rows}
    line = json.dumps(out)
    if not a.no_write:
        with open(os.path.join(ROOT, "profiles", "cluster_average_bench.json"), "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
