"""The ANI metrics (hg_ctx_set_ani_metric) side by side on the thresholded 10 000 x 10 000 GEMM.  Prints one JSON line.

Inputs: bench.clustered_hvs (two distinct sets with the bench's hit structure) and tests/containment_ref.fragment_hvs (members
that keep 5 .. 100 % of a parent's hashes).  Per input and metric the threshold is chosen so that the hit count is that of
HG_ANI_MASH at --ani_th (the value at the same rank of the metric's full matrix), and the calls alternate metric by metric,
--steps each after --warmup: the line carries the median wall ms of hg_dist_dev (R x Q, and the symmetric form of the first
set for the symmetric metrics), the hit counts, the thresholds, hg_ctx_last_dist_path, and hg_cluster_dev at --ani_th.
Kernel times: run it under `rocprofv3 --kernel-trace --stats`.

    python tools/containment_bench.py [--n 10000 --ani_th 95 --steps 20 --warmup 3] [--mash-only --root <tree>]

--mash-only --root <tree>: HG_ANI_MASH only, with the package of another tree (a build of a library without the metrics).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10000)
    ap.add_argument("--ani_th", type=float, default=95.0)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--mash-only", action="store_true")
    ap.add_argument("--root", default=ROOT)
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, a.root)
    import numpy as np
    import torch
    import hypergen_amd as hg
    import bench
    dev = torch.device("cuda:0")
    n, D = a.n, 4096
    metrics = (0,) if a.mash_only else (0, 1, 2)
    inputs = {"clustered": (bench.clustered_hvs(n, 0, dev), bench.clustered_hvs(n, 0, dev, salt=1))}
    if not a.mash_only:
        import containment_ref as cr
        hv, _, _ = cr.fragment_hvs(2 * n, D=D, seed=9)
        t = torch.from_numpy(hv).to(dev)
        inputs["fragments"] = (t[:n].contiguous(), t[n:].contiguous())
    cap = 40_000_000
    hits = torch.empty(3 * cap, dtype=torch.int32, device=dev)
    out = {"n": n, "ani_th": a.ani_th, "steps": a.steps, "library": "this tree" if a.root == ROOT else "the tree at --root"}
    with hg.Context(0) as ctx:
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        for name, (r, q) in inputs.items():
            rn, qn = (r.int() ** 2).sum(1).int(), (q.int() ** 2).sum(1).int()
            torch.cuda.synchronize()
            th, in_full = {0: a.ani_th}, {}
            if not a.mash_only:  # thresholds at the Mash hit count's rank; in_full: pairs >= the threshold in the full matrix
                full = torch.empty((n, n), dtype=torch.float32, device=dev)
                for m in (0, 1, 2):
                    ctx.set_ani_metric(m)
                    ctx.dist_full_dev(r.data_ptr(), rn.data_ptr(), n, q.data_ptr(), qn.data_ptr(), n, D, 21, full.data_ptr())
                    ctx.sync()
                    if m == 0:
                        k = int((full >= a.ani_th).sum())
                    else:
                        th[m] = float(torch.sort(full.ravel(), descending=True).values[max(k, 1) - 1])
                    in_full[m] = int((full >= th[m]).sum())
                ctx.set_ani_metric(0)
                del full
            forms = [("rq", False)] + ([("sym", True)] if name == "clustered" else [])
            for form, sym in forms:
                ms = {m: [] for m in metrics if not (sym and m == 1)}
                res = {}

                def call(m):
                    if not a.mash_only:
                        ctx.set_ani_metric(m)
                    qq, qqn = (r, rn) if sym else (q, qn)
                    t0 = time.perf_counter()
                    f, st = ctx.dist_dev(r.data_ptr(), rn.data_ptr(), n, qq.data_ptr(), qqn.data_ptr(), n, D, 21, sym, th[m],
                                         hits.data_ptr(), cap)
                    dt = (time.perf_counter() - t0) * 1e3
                    assert st == 0
                    res[m] = (f, ctx.last_dist_path(), ctx.last_kernel("dist"))
                    return dt
                for _ in range(a.warmup):
                    for m in ms:
                        call(m)
                for _ in range(a.steps):
                    for m in ms:
                        ms[m].append(call(m))
                for m in ms:
                    key = "%s_%s_%s" % (name, form, ("mash", "containment", "max_containment")[m])
                    out[key] = {"ms": round(float(np.median(ms[m])), 4), "hits": res[m][0], "ani_th": th[m],
                                "dist_path": res[m][1], "kernel": res[m][2]}
                    if form == "rq" and m in in_full:
                        out[key]["hits_in_full_matrix"] = in_full[m]
        # clustering at ani_th
        r = inputs["clustered"][0]
        rn = (r.int() ** 2).sum(1).int()
        rep = torch.empty(n, dtype=torch.int32, device=dev)
        cl = torch.empty(n, dtype=torch.int32, device=dev)
        for m in ((0,) if a.mash_only else (0, 2)):
            if not a.mash_only:
                ctx.set_ani_metric(m)
            ts = []
            for i in range(a.warmup + a.steps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                nc = ctx.cluster_dev(r.data_ptr(), rn.data_ptr(), n, D, rep.data_ptr(), cl.data_ptr(), 21, a.ani_th)
                if i >= a.warmup:
                    ts.append((time.perf_counter() - t0) * 1e3)
            out["cluster_%s" % ("mash", "", "max_containment")[m]] = {"ms": round(float(np.median(ts)), 4), "clusters": nc}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
