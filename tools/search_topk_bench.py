"""`search` two ways in one process: the bounded-memory selection (hg_search_topk_dev) against the hit-list route
(hg_dist_dev followed by hg_topk_per_query_dev).  Prints one JSON line.

Inputs: bench.clustered_hvs (two distinct sets with the bench's hit structure: about 1 % of the pairs pass 85).  Per shape,
threshold and k both routes are warmed up and then alternate for --rounds rounds; the line carries every round's wall ms
(call to results final on the device), the median, min and max, the ratio of the medians (new / old: above 1 = the new path
is slower), the hit count the old route had to hold, and whether the two outputs were equal.  `select_bytes` is what the
selection kernels of ONE new call read (R * Q * 4, the matrix blocks): divide it by the kernel's time from a separate
`rocprofv3 --kernel-trace --stats` run (--only new --shapes ... keeps that run to one route) for its bytes per second.

    python tools/search_topk_bench.py [--rounds 3 --warmup 1] [--shapes 10000x10000,100000x1000,100000x10] [--only new|old]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--shapes", default="10000x10000,100000x1000,100000x10")
    ap.add_argument("--only", choices=("new", "old"), default=None)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import hypergen_amd as hg
    import bench
    dev = torch.device("cuda:0")
    D = 4096
    out = {"rounds": a.rounds, "warmup": a.warmup, "cases": []}
    with hg.Context(0) as ctx:
        for shape in a.shapes.split(","):
            R, Q = (int(x) for x in shape.split("x"))
            r, q = bench.clustered_hvs(R, 0, dev), bench.clustered_hvs(Q, 0, dev, salt=1)
            rn, qn = (r.int() ** 2).sum(1).int(), (q.int() ** 2).sum(1).int()
            # (the old route at th = 0 holds every pair: 10^8 hits at 10 000 x 10 000; the larger shapes run at 85 only)
            for th in ((85.0, 0.0) if R * Q <= 10 ** 8 and Q >= 10000 else (85.0,)):
                cap = R * Q if th == 0.0 else max(1 << 20, R * Q // 8)
                hits = torch.empty(3 * cap, dtype=torch.int32, device=dev) if a.only != "new" else None
                for k in (1, 10):
                    res = [torch.zeros(Q * k * 3, dtype=torch.int32, device=dev) for _ in range(2)]
                    cnt = [torch.zeros(Q, dtype=torch.int32, device=dev) for _ in range(2)]
                    torch.cuda.synchronize()
                    found = [0]

                    def new():
                        t0 = time.perf_counter()
                        ctx.search_topk_dev(r.data_ptr(), rn.data_ptr(), R, q.data_ptr(), qn.data_ptr(), Q, D, 21, th, k,
                                            res[0].data_ptr(), cnt[0].data_ptr())
                        ctx.sync()
                        return (time.perf_counter() - t0) * 1e3

                    def old():
                        t0 = time.perf_counter()
                        f, st = ctx.dist_dev(r.data_ptr(), rn.data_ptr(), R, q.data_ptr(), qn.data_ptr(), Q, D, 21, False, th,
                                             hits.data_ptr(), cap)
                        assert st == 0, st
                        ctx.topk_per_query_dev(hits.data_ptr(), f, Q, k, res[1].data_ptr(), cnt[1].data_ptr())
                        ctx.sync()
                        found[0] = f
                        return (time.perf_counter() - t0) * 1e3

                    routes = [(n, f) for n, f in (("new", new), ("old", old)) if a.only in (None, n)]
                    for _ in range(a.warmup):
                        for _, f in routes:
                            f()
                    ms = {n: [] for n, _ in routes}
                    for _ in range(a.rounds):
                        for n, f in routes:
                            ms[n].append(f())
                    case = {"R": R, "Q": Q, "ani_th": th, "k": k, "select_bytes": R * Q * 4}
                    for n in ms:
                        case[n + "_ms"] = [round(x, 3) for x in ms[n]]
                        case[n + "_ms_median"] = round(float(np.median(ms[n])), 3)
                        case[n + "_ms_min_max"] = [round(min(ms[n]), 3), round(max(ms[n]), 3)]
                    if len(ms) == 2:
                        case["ratio_new_over_old"] = round(case["new_ms_median"] / case["old_ms_median"], 3)
                        case["old_hits"] = int(found[0])
                        case["old_hit_list_bytes"] = int(found[0]) * 12
                        case["equal"] = bool(torch.equal(res[0], res[1]) and torch.equal(cnt[0], cnt[1]))
                    out["cases"].append(case)
                del hits
            del r, q
            torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
