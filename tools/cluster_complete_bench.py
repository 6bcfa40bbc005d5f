"""hg_cluster_complete_dev, with its default rescan rule and with "complete_rescan" = "all", against hg_cluster_average_dev
and against hg_dist_full_dev of the same sketches (bench.clustered_hvs: clusters of 100 members, ~96-97 % ANI inside a
cluster): what complete linkage -- the dense matrix of u32 minima, half of average linkage's, filled from blocks of the ANI
matrix, and four launches per round over it -- costs on top of the comparison it needs anyway, what scanning only the rows
a merge invalidated saves, and how the scheme compares with average linkage.  Two thresholds per size: 95 and the median
within-cluster ANI (read from hg_dist_full_dev of rows 0..299).  The four legs alternate in one process, --rounds times;
each leg of a round is the median wall ms of --steps calls (every call returns with its results final).  Prints one JSON
line and writes it to profiles/cluster_complete_bench.json: per size and threshold the clusters and the rounds of both
schemes, how many clusters hg_cluster_stats_dev counts as not separated under each (highest outside ANI >= lowest within
ANI, clusters of two or more), the matrix held and per leg the median of the rounds with min and max.  No ratio is a pass
condition.

    python tools/cluster_complete_bench.py [--n 10000 30000] [--rounds 3 --steps 3 --warmup 1] [--no-write]
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


def not_separated(c, hg, torch, hv, n2, n, D, cl, k):
    """clusters of two or more whose nearest outside sketch is as close as their two least similar members"""
    import numpy as np
    d_stat = torch.zeros(max(k, 1) * 48, dtype=torch.uint8, device=hv.device)
    torch.cuda.synchronize()
    c.cluster_stats_dev(hv.data_ptr(), n2.data_ptr(), n, D, cl.data_ptr(), k, None, d_stat.data_ptr(), 21)
    c.sync()
    s = d_stat.cpu().numpy()[:k * 48].view(hg.CLUSTER_STAT_DTYPE)
    both = (s["size"] >= 2) & (s["outside_idx"] != hg.STATS_NONE)
    return int((both & (s["outside_max"] >= s["within_min"])).sum()), int((s["size"] >= 2).sum())


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

        def complete(key):
            def run():
                c.set_debug("complete_rescan", "all" if key == "complete_rescan_all" else "")
                res[key + "_clusters"] = c.cluster_complete_dev(hv.data_ptr(), n2.data_ptr(), n, D, rep.data_ptr(), cl.data_ptr(),
                                                                 None, None, None, 21, th)
                res[key + "_rounds"] = c.cluster_complete_rounds()
                c.set_debug("complete_rescan", "")
            return run

        def average():
            res["average_clusters"] = c.cluster_average_dev(hv.data_ptr(), n2.data_ptr(), n, D, rep.data_ptr(), cl.data_ptr(),
                                                            None, None, None, 21, th)
            res["average_rounds"] = c.cluster_average_rounds()

        legs = {"dist_full": dist_full, "complete": complete("complete"), "complete_rescan_all": complete("complete_rescan_all"),
                "average": average}
        for fn in legs.values():
            for _ in range(a.warmup):
                fn()
        per = {k: [] for k in legs}
        for _ in range(a.rounds):
            for k, fn in legs.items():
                per[k].append(median_ms(fn, a.steps))
        # separation under each scheme, from the product's own statistics (cl holds the assignment of the call before)
        for k in ("average", "complete"):
            legs[k]()
            bad, several = not_separated(c, hg, torch, hv, n2, n, D, cl, res[k + "_clusters"])
            res[k + "_not_separated"], res[k + "_clusters_of_two_or_more"] = bad, several
        row = {"n": n, "ani_th": round(th, 4), **res, "matrix_mb": round(n * ((n + 3) // 4 * 4) * 4 / 1e6, 1)}
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
            rows += measure_one(c, hg, torch, bench, n, a)
    out = {"bench": "cluster_complete", "status": "measured", "rounds": a.rounds,
           "steps": a.steps, "launches_per_round": 4, "cases": rows}
    line = json.dumps(out)
    if not a.no_write:
        with open(os.path.join(ROOT, "profiles", "cluster_complete_bench.json"), "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
