"""hg_ani_pairs_dev beside the comparison that produced -- or would have to produce -- its list.  Prints one JSON line.

Two cases, D = 4096, all four columns:
  hits   : --n clustered HVs against a second such set (bench.clustered_hvs), thresholded at the rank that gives --hits pairs
           (the dist bench's about 1.29 M).  The list in three orders: "dist" as hg_dist_dev left it, "sorted" after
           hg_sort_ani_hits_dev (the order `dist --columns` uses), "by_ref" sorted by ref_idx, then qry_idx (the bound of what
           locality can give).  Beside them hg_dist_dev + hg_sort_ani_hits_dev alone: the share --columns adds is visible.
  listed : --listed random pairs of --big sketches (`dist --pairs` with a short list against a large database), in the order
           listed, in hg_sort_ani_hits_dev's order and by ref_idx; beside them hg_dist_dev + the sort of the whole --big x --big
           matrix at a threshold that yields about as many hits -- the only route to those values without the call.
Every figure is the wall time of the call plus hg_ctx_sync, the median of --rounds alternating rounds in one process after
--warmup rounds, with the minimum and maximum beside it; gb_per_s = n_pairs x 4 x hv_d bytes (both rows of every pair) per
second of the median.  The yardstick for that rate is the gathered-row range of the hardware, not a pass condition.

    python tools/ani_pairs_bench.py [--n 10000 --hits 1290000 --big 100000 --listed 10000 --rounds 3 --warmup 1]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D, K = 4096, 21


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10000)
    ap.add_argument("--hits", type=int, default=1_290_000)
    ap.add_argument("--big", type=int, default=100_000)
    ap.add_argument("--listed", type=int, default=10_000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import hypergen_amd as hg
    import bench
    dev = torch.device("cuda:0")
    out = {"hv_d": D, "ksize": K, "columns": 15, "rounds": a.rounds, "source_stamp": hg.source_stamp()}

    def stats(ms, n_pairs=None):
        s = {"ms": round(float(np.median(ms)), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}
        if n_pairs:
            s["gb_per_s"] = round(n_pairs * 4 * D / (s["ms"] * 1e-3) / 1e9, 1)
        return s

    def by_ref(lst, n, Q):
        """the records of a device list (3 int32 each) ordered by ref_idx, then qry_idx"""
        rec = lst[: 3 * n].view(n, 3)
        key = (rec[:, 0].long() & 0xFFFFFFFF) * Q + (rec[:, 1].long() & 0xFFFFFFFF)
        return rec[torch.argsort(key)].contiguous().view(-1)

    with hg.Context(0) as ctx:
        ctx.set_stream(torch.cuda.current_stream().cuda_stream)

        def run_case(r, q, th, lists, cap):
            """alternating rounds of hg_dist_dev + sort at `th` and hg_ani_pairs_dev on every list of `lists` {name: (tensor, n)}"""
            R, Q = r.shape[0], q.shape[0]
            rn, qn = (r.int() ** 2).sum(1).int(), (q.int() ** 2).sum(1).int()
            scratch = torch.empty(3 * cap, dtype=torch.int32, device=dev)
            n_max = max(n for _, n in lists.values())
            ani = torch.empty(4 * n_max, dtype=torch.float32, device=dev)
            ms = {k: [] for k in ["dist_sort"] + list(lists)}
            found = 0
            for rnd in range(a.warmup + a.rounds):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                found, st = ctx.dist_dev(r.data_ptr(), rn.data_ptr(), R, q.data_ptr(), qn.data_ptr(), Q, D, K, False, th, scratch.data_ptr(), cap)
                ctx.sort_ani_hits_dev(scratch.data_ptr(), found, Q)
                ctx.sync()
                dt = (time.perf_counter() - t0) * 1e3
                assert st == 0, "hit buffer too small: %d hits" % found
                if rnd >= a.warmup:
                    ms["dist_sort"].append(dt)
                for name, (lst, n) in lists.items():
                    t0 = time.perf_counter()
                    ctx.ani_pairs_dev(r.data_ptr(), rn.data_ptr(), R, q.data_ptr(), qn.data_ptr(), Q, D, K, lst.data_ptr(), n, 15, ani.data_ptr())
                    ctx.sync()
                    dt = (time.perf_counter() - t0) * 1e3
                    if rnd >= a.warmup:
                        ms[name].append(dt)
            res = {"dist_sort": dict(stats(ms["dist_sort"]), hits=found, ani_th=th, kernel_note="hg_dist_dev + hg_sort_ani_hits_dev")}
            for name, (_, n) in lists.items():
                res[name] = dict(stats(ms[name], n), n_pairs=n)
            return res

        # ---- case 1: the hit list of the dist bench's comparison -------------------------------------------------------------
        n = a.n
        r, q = bench.clustered_hvs(n, 0, dev), bench.clustered_hvs(n, 0, dev, salt=1)
        rn, qn = (r.int() ** 2).sum(1).int(), (q.int() ** 2).sum(1).int()
        full = torch.empty((n, n), dtype=torch.float32, device=dev)
        ctx.dist_full_dev(r.data_ptr(), rn.data_ptr(), n, q.data_ptr(), qn.data_ptr(), n, D, K, full.data_ptr())
        ctx.sync()
        want = min(a.hits, n * n)
        th = float(torch.sort(full.ravel(), descending=True).values[want - 1])
        cap = int((full >= th).sum()) + 1024
        del full
        lst = torch.empty(3 * cap, dtype=torch.int32, device=dev)
        found, st = ctx.dist_dev(r.data_ptr(), rn.data_ptr(), n, q.data_ptr(), qn.data_ptr(), n, D, K, False, th, lst.data_ptr(), cap)
        assert st == 0
        as_left = lst[: 3 * found].clone()
        ctx.sort_ani_hits_dev(lst.data_ptr(), found, n)
        ctx.sync()
        lists = {"dist": (as_left, found), "sorted": (lst, found), "by_ref": (by_ref(lst, found, n), found)}
        out["hits"] = run_case(r, q, th, lists, cap)
        out["hits"].update(R=n, Q=n)
        del r, q, lst, as_left, lists
        # ---- case 2: a short list against a large database ---------------------------------------------------------------------
        B, n_l = a.big, a.listed
        r = torch.cat([bench.clustered_hvs(min(10000, B - i), i, dev) for i in range(0, B, 10000)])
        q = torch.cat([bench.clustered_hvs(min(10000, B - i), i, dev, salt=1) for i in range(0, B, 10000)])
        rn, qn = (r.int() ** 2).sum(1).int(), (q.int() ** 2).sum(1).int()
        g = torch.Generator(device=dev)
        g.manual_seed(0x50414952)
        rec = torch.zeros((n_l, 3), dtype=torch.int32, device=dev)
        rec[:, 0] = torch.randint(0, B, (n_l,), generator=g, device=dev, dtype=torch.int32)
        # (half of the list within the reference's cluster of 100, as a list of candidate pairs would be; half anywhere)
        near = (rec[:, 0] // 100) * 100 + torch.randint(0, 100, (n_l,), generator=g, device=dev, dtype=torch.int32)
        far = torch.randint(0, B, (n_l,), generator=g, device=dev, dtype=torch.int32)
        rec[:, 1] = torch.where(torch.arange(n_l, device=dev) % 2 == 0, torch.minimum(near, torch.tensor(B - 1, dtype=torch.int32, device=dev)), far)
        listed = rec.view(-1).contiguous()
        ani = torch.empty(n_l, dtype=torch.float32, device=dev)
        ctx.ani_pairs_dev(r.data_ptr(), rn.data_ptr(), B, q.data_ptr(), qn.data_ptr(), B, D, K, listed.data_ptr(), n_l, 1, ani.data_ptr())
        with_ani = rec.clone()
        with_ani[:, 2] = ani.view(torch.int32)
        ordered = with_ani.view(-1).contiguous()
        ctx.sort_ani_hits_dev(ordered.data_ptr(), n_l, B)
        ctx.sync()
        # the threshold at which the whole comparison reports about as many hits as the list has pairs: bisected on the hit
        # count of hg_dist_dev itself (the B x B matrix is too large to sort)
        cap = 64 * n_l + 1024
        scratch = torch.empty(3 * cap, dtype=torch.int32, device=dev)
        lo, hi, th = 90.0, 100.0, 99.0
        for _ in range(24):
            th = (lo + hi) / 2
            found, st = ctx.dist_dev(r.data_ptr(), rn.data_ptr(), B, q.data_ptr(), qn.data_ptr(), B, D, K, False, th, scratch.data_ptr(), cap)
            if st == 0 and 0.9 * n_l <= found <= 1.1 * n_l:
                break
            if found > n_l:
                lo = th
            else:
                hi = th
        del scratch
        lists = {"listed": (listed, n_l), "sorted": (ordered, n_l), "by_ref": (by_ref(listed, n_l, B), n_l)}
        out["listed"] = run_case(r, q, th, lists, cap)
        out["listed"].update(R=B, Q=B)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
