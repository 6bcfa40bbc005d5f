"""hg_cluster_stats_dev against hg_dist_full_dev run over the same row blocks of the same sketches (bench.clustered_hvs:
clusters of 100 members, ~96-97 % ANI inside a cluster): what the statistics -- cluster_stats_rows_kernel over every block
and the fold of the node records -- cost on top of the comparison they need (the matrix in full, not as a triangle: every
row has its own minimum and maximum).  Two assignments per size: hg_cluster_dev at 95 and hg_cluster_average_dev at the
median within-cluster ANI (read from hg_dist_full_dev of rows 0..299).  The two legs alternate in one process, --rounds
times; each leg of a round is the median wall ms of --steps calls (every call returns with its results final).  Prints one
JSON line and writes it to profiles/cluster_stats_bench.json.  No ratio is a pass condition.

    python tools/cluster_stats_bench.py [--n 10000 30000] [--rounds 3 --steps 3 --warmup 1] [--no-write]

The rows kernel's rate comes from a run of its own under the profiler, which writes nothing,

    rocprofv3 --kernel-trace --stats -d DIR -o stats --output-format csv -- python tools/cluster_stats_bench.py --profiled 10000

and is merged into the committed file afterwards:

    python tools/cluster_stats_bench.py --merge-kernel-stats DIR/.../stats_kernel_stats.csv --profiled 10000
"""
import argparse
import csv
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "cluster_stats_bench.json")
BLOCK_BYTES = 256 << 20  # HG_SEARCH_BLOCK_BYTES
PROFILED_CALLS = 5


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


def setup(c, torch, bench, n):
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
    return hv, n2, D, float(np.median(m[i, j][i // 100 == j // 100]))


def assignments(c, torch, hv, n2, D, n, band):
    out = []
    for how, th in (("single", 95.0), ("average", band)):
        rep = torch.empty(n, dtype=torch.int32, device=hv.device)
        cl = torch.empty(n, dtype=torch.int32, device=hv.device)
        torch.cuda.synchronize()
        fn = c.cluster_dev if how == "single" else c.cluster_average_dev
        nc = fn(hv.data_ptr(), n2.data_ptr(), n, D, rep.data_ptr(), cl.data_ptr(), ksize=21, ani_th=th)
        out.append((how, th, cl, nc))
    return out


def measure_one(c, torch, bench, n, a):
    import numpy as np
    import cluster_stats_ref as st
    hv, n2, D, band = setup(c, torch, bench, n)
    rb = max(1, min(n, BLOCK_BYTES // (4 * n)))
    blk = torch.empty(rb * n, dtype=torch.float32, device=hv.device)
    rows = []
    for how, th, cl, nc in assignments(c, torch, hv, n2, D, n, band):
        d_stat = torch.zeros(nc * 48, dtype=torch.uint8, device=hv.device)
        torch.cuda.synchronize()

        def dist_blocks():
            for r0 in range(0, n, rb):
                r = min(rb, n - r0)
                c.dist_full_dev(hv.data_ptr() + 2 * r0 * D, n2.data_ptr() + 4 * r0, r, hv.data_ptr(), n2.data_ptr(), n, D, 21, blk.data_ptr())
            c.sync()

        def stats():
            c.cluster_stats_dev(hv.data_ptr(), n2.data_ptr(), n, D, cl.data_ptr(), nc, None, d_stat.data_ptr(), 21)

        legs = {"dist_full_blocks": dist_blocks, "stats": stats}
        for fn in legs.values():
            for _ in range(a.warmup):
                fn()
        per = {k: [] for k in legs}
        for _ in range(a.rounds):
            for k, fn in legs.items():
                per[k].append(median_ms(fn, a.steps))
        s = d_stat.cpu().numpy().view(st.CLUSTER_DTYPE)
        pairs = s["size"] >= 2
        row = {"n": n, "assignment": how, "ani_th": round(th, 4), "clusters": int(nc), "block_rows": rb,
               "not_separated": st.not_separated(s),
               "lowest_within_min": round(float(s["within_min"][pairs].min()) / 1000.0, 3) if pairs.any() else None}
        for k in legs:
            row[k] = summary(per[k])
        row["stats_over_dist"] = round(row["stats"]["median_ms"] / row["dist_full_blocks"]["median_ms"], 3)
        rows.append(row)
    return rows


def profiled(c, torch, bench, n):
    hv, n2, D, band = setup(c, torch, bench, n)
    how, th, cl, nc = assignments(c, torch, hv, n2, D, n, band)[0]
    d_stat = torch.zeros(nc * 48, dtype=torch.uint8, device=hv.device)
    torch.cuda.synchronize()
    for _ in range(PROFILED_CALLS):
        c.cluster_stats_dev(hv.data_ptr(), n2.data_ptr(), n, D, cl.data_ptr(), nc, None, d_stat.data_ptr(), 21)


def merge_kernel_stats(path, n):
    total_ns = calls = None
    with open(path) as f:
        for r in csv.DictReader(f):
            if "cluster_stats_rows_kernel" in r.get("Name", ""):
                total_ns, calls = float(r["TotalDurationNs"]), int(r["Calls"])
    if total_ns is None:
        sys.exit("no cluster_stats_rows_kernel row in %s" % path)
    matrix_bytes = PROFILED_CALLS * n * n * 4  # the floats of the matrix; the ids are re-read from cache
    out = json.load(open(OUT))
    out["rows_kernel"] = {"n": n, "launches": calls, "total_ms": round(total_ns / 1e6, 3),
                          "matrix_bytes_per_s": round(matrix_bytes / (total_ns / 1e9), -6),
                          "source": "rocprofv3 --kernel-trace --stats of %d hg_cluster_stats_dev calls, a run of its own" % PROFILED_CALLS}
    line = json.dumps(out)
    with open(OUT, "w") as f:
        f.write(line + "\n")
    print(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[10_000, 30_000])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--no-write", action="store_true")
    ap.add_argument("--profiled", type=int, default=0, help="only run the calls a profiler traces, at this size")
    ap.add_argument("--merge-kernel-stats", default=None, help="a rocprofv3 kernel stats CSV of a --profiled run")
    a = ap.parse_args()
    if a.merge_kernel_stats:
        return merge_kernel_stats(a.merge_kernel_stats, a.profiled or 10_000)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch
    import hypergen_amd as hg
    import bench
    with hg.Context(0) as c:
        if a.profiled:
            return profiled(c, torch, bench, a.profiled)
        rows = []
        for n in a.n:
            rows += measure_one(c, torch, bench, n, a)
    out = {"bench": "cluster_stats", "status": "measured", "rounds": a.rounds, "steps": a.steps, "cases": rows}
    line = json.dumps(out)
    if not a.no_write:
        with open(OUT, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
