"""hg_nj_dev against hg_cluster_average_dev and hg_dist_full_dev of the same sketches (bench.clustered_hvs, the generator of
tools/cluster_complete_bench.py: clusters of 100 members, ~96-97 % ANI inside a cluster): what the neighbour-joining tree
-- the dense u32 matrix filled from blocks of the ANI matrix, then n - 2 rounds of three launches and the last join, all
queued ahead -- costs on top of the comparison it needs anyway, and next to the other tree-shaped result the library has,
the UPGMA dendrogram.  The three legs alternate in one process, --rounds times; each leg of a round is the median wall ms
of --steps calls (every call returns with its results final).  Prints one JSON line and writes it to
profiles/nj_bench.json: per size the join count, the share of joins with a negative branch length, the matrix held and
per leg the median of the rounds with min and max.  No ratio is a pass condition.

    python tools/nj_bench.py [--n 10000 30000] [--rounds 3 --steps 1 --warmup 1] [--no-write]
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


def measure_one(c, hg, torch, bench, n, a):
    dev = torch.device("cuda:0")
    hv = bench.clustered_hvs(n, 0, dev)
    n2 = (hv.int() ** 2).sum(1).int()
    D = hv.shape[1]
    full = torch.empty(n * n, dtype=torch.float32, device=dev)
    rep = torch.empty(n, dtype=torch.int32, device=dev)
    cl = torch.empty(n, dtype=torch.int32, device=dev)
    joins = torch.zeros((n - 1) * 24, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    res = {}

    def dist_full():
        c.dist_full_dev(hv.data_ptr(), n2.data_ptr(), n, hv.data_ptr(), n2.data_ptr(), n, D, 21, full.data_ptr())
        c.sync()

    def nj():
        res["joins"] = c.nj_dev(hv.data_ptr(), n2.data_ptr(), n, D, joins.data_ptr(), 21)

    def average():
        res["average_clusters"] = c.cluster_average_dev(hv.data_ptr(), n2.data_ptr(), n, D, rep.data_ptr(), cl.data_ptr(), None, None, None,
                                                        21, 95.0)
        res["average_rounds"] = c.cluster_average_rounds()

    legs = {"dist_full": dist_full, "nj": nj, "average": average}
    for name, fn in legs.items():
        for _ in range(a.warmup):
            fn()
        print("n %d: %s warmed up" % (n, name), file=sys.stderr, flush=True)
    per = {k: [] for k in legs}
    for r in range(a.rounds):
        for k, fn in legs.items():
            per[k].append(median_ms(fn, a.steps))
        print("n %d: round %d done" % (n, r + 1), file=sys.stderr, flush=True)
    j = joins.cpu().numpy().view(hg.NJ_JOIN_DTYPE)
    negative = int(((j["len_a"] < 0) | (j["len_b"] < 0)).sum())
    row = {"n": n, **res, "negative_joins": negative, "negative_share": round(negative / max(len(j), 1), 4),
           "matrix_mb": round(n * ((n + 3) // 4 * 4) * 4 / 1e6, 1)}
    for k in legs:
        row[k] = summary(per[k])
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[10_000, 30_000])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=1)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--no-write", action="store_true")
    a = ap.parse_args()
    import torch
    import hypergen_amd as hg
    import bench
    rows = []
    with hg.Context(0) as c:
        for n in a.n:
            rows.append(measure_one(c, hg, torch, bench, n, a))
    out = {"bench": "nj", "status": "measured", "rounds": a.rounds, "steps": a.steps, "launches_per_round": 3, "cases": rows}
    line = json.dumps(out)
    if not a.no_write:
        with open(os.path.join(ROOT, "profiles", "nj_bench.json"), "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
