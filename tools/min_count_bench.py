"""The sketch step on raw READ sets, with and without hg_sketch_params.min_count.  Read sets are made on the device with torch
(windows of a seeded genome tensor, substitutions at `--err`, half of the reads reverse-complemented, an N in front of each
read): `--sets` read sets of `--genome` bp at `--cov`-fold coverage, resident as ASCII, k = 21, scaled = 1 500.  For every m of
`--m` the whole batch is sketched `--steps` times warm; per step: the wall ms (call + hg_ctx_sync), the read-Gbp/s that is --
an END-TO-END figure of the resident step --, and the device ms of the k-mer, sort and encode classes from hg_ctx_timings
(a second pass with timing on).  Prints one JSON line.

    python tools/min_count_bench.py [--sets 32 --genome 5000000 --cov 30 --steps 20 --warmup 3 --m 1,2]
    python tools/min_count_bench.py --parent-tree <a built checkout of the commit to compare with> [--rounds 3]

With --parent-tree the measurement runs as child processes, alternating between that checkout (m = 1 only: it may not know the
field) and this one (`--m`), `--rounds` times, and the line carries every run, the medians, the spread of the repeated runs
and the ratios: sort(m = 2) / sort(parent, m = 1), kmer and encode at m = 2 against m = 1.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", type=int, default=32)
    ap.add_argument("--genome", type=int, default=5_000_000)
    ap.add_argument("--cov", type=int, default=30)
    ap.add_argument("--read", type=int, default=150)
    ap.add_argument("--err", type=float, default=0.01)
    ap.add_argument("--scaled", type=int, default=1500)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--m", default="1,2")
    ap.add_argument("--tree", default=ROOT, help="checkout whose library is measured (default: this one)")
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    return ap.parse_args()


def read_sets(a, torch, dev):
    """(buffer, offsets, lens): the read sets, one after the other at multiples of 16"""
    rl, n = a.read, a.genome * a.cov // a.read
    stride = (n * (rl + 1) + 15) // 16 * 16
    buf = torch.zeros(a.sets * stride + 64, dtype=torch.uint8, device=dev)
    lut = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=dev)
    ar = torch.arange(rl, device=dev)
    for s in range(a.sets):
        gen = torch.Generator(device=dev)
        gen.manual_seed(1000 + s)
        g = torch.randint(0, 4, (a.genome,), dtype=torch.uint8, device=dev, generator=gen)
        out = buf[s * stride: s * stride + n * (rl + 1)].view(n, rl + 1)
        out[:, 0] = ord("N")
        for lo in range(0, n, 1 << 18):  # (in slices: the index tensor of a whole set would take 1.2 GB)
            hi = min(n, lo + (1 << 18))
            starts = torch.randint(0, a.genome - rl, (hi - lo,), device=dev, generator=gen)
            r = g[starts[:, None] + ar]
            sub = torch.rand((hi - lo, rl), device=dev, generator=gen) < a.err
            r = torch.where(sub, (r + torch.randint(1, 4, r.shape, dtype=torch.uint8, device=dev, generator=gen)) % 4, r)
            rc = torch.rand((hi - lo,), device=dev, generator=gen) < 0.5
            r = torch.where(rc[:, None], 3 - r.flip(1), r)
            out[lo:hi, 1:] = lut[r.long()]
    import numpy as np
    return buf, np.arange(a.sets, dtype=np.uint64) * stride, np.full(a.sets, n * (rl + 1), np.uint64)


def measure(a):
    sys.path.insert(0, a.tree)
    import torch
    import numpy as np
    import hypergen_amd as hg
    dev = torch.device("cuda:0")
    buf, offs, lens = read_sets(a, torch, dev)
    torch.cuda.synchronize()
    bases = float(a.sets) * (a.genome * a.cov // a.read) * a.read
    res = {"tree": os.path.abspath(a.tree), "version": hg.lib().hg_version().decode(), "sets": a.sets, "genome_bp": a.genome,
           "coverage": a.cov, "read_len": a.read, "err": a.err, "scaled": a.scaled, "steps": a.steps, "read_gbp": bases / 1e9, "m": {}}
    hv = torch.empty((a.sets, 4096), dtype=torch.int16, device=dev)
    n2 = torch.empty(a.sets, dtype=torch.int32, device=dev)
    nh = torch.empty(a.sets, dtype=torch.int32, device=dev)
    with hg.Context(0) as c:
        for m in [int(x) for x in a.m.split(",")]:
            p = hg.default_params(scaled=a.scaled)
            if m > 1:
                p.min_count = m

            def step():
                c.sketch_batch_dev(buf.data_ptr(), offs, lens, p, hv.data_ptr(), n2.data_ptr(), nh.data_ptr())
                c.sync()

            for _ in range(a.warmup):
                step()
            wall = []
            for _ in range(a.steps):
                t0 = time.perf_counter()
                step()
                wall.append((time.perf_counter() - t0) * 1e3)
            wall.sort()
            c.enable_timing(True)
            step()
            c.timings()
            for _ in range(a.steps):
                step()
            t = c.timings()
            c.enable_timing(False)
            med = wall[len(wall) // 2]
            res["m"][str(m)] = {"wall_ms": round(med, 3), "wall_ms_min": round(wall[0], 3), "end_to_end_read_gbp_per_s": round(bases / 1e6 / med, 1),
                                "kmer_ms": round(t["kmer"][0] / a.steps, 4), "sort_ms": round(t["sort"][0] / a.steps, 4),
                                "encode_ms": round(t["encode"][0] / a.steps, 4), "sort_kernels": c.last_kernel("sort"),
                                "nhash_mean": float(nh.cpu().numpy().view(np.uint32).mean()), "step_counts": c.sketch_step_counts()}
    return res


def compare(a):
    def child(tree, m):
        cmd = [sys.executable, os.path.abspath(__file__), "--tree", tree, "--m", m]
        for k in ("sets", "genome", "cov", "read", "err", "scaled", "steps", "warmup"):
            cmd += ["--" + k, str(getattr(a, k))]
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        if out.returncode != 0:
            raise SystemExit("child failed (%s):\n%s" % (tree, out.stderr[-2000:]))
        return json.loads(out.stdout.strip().splitlines()[-1])

    runs = {"parent": [], "branch": []}
    for _ in range(a.rounds):
        runs["parent"].append(child(a.parent_tree, "1"))
        runs["branch"].append(child(ROOT, a.m))

    def med(xs):
        xs = sorted(xs)
        return xs[len(xs) // 2]

    def col(side, m, key):
        return [r["m"][m][key] for r in runs[side]]

    out = {"what": "sketch step on read sets: parent commit (m = 1) against this tree, alternating child processes", "rounds": a.rounds,
           "config": {k: runs["branch"][0][k] for k in ("sets", "genome_bp", "coverage", "read_len", "err", "scaled", "steps", "read_gbp")},
           "runs": runs, "median": {}, "spread": {}}
    for side, ms in (("parent", ["1"]), ("branch", a.m.split(","))):
        for m in ms:
            for key in ("wall_ms", "kmer_ms", "sort_ms", "encode_ms", "end_to_end_read_gbp_per_s"):
                v = col(side, m, key)
                out["median"]["%s.m%s.%s" % (side, m, key)] = med(v)
                out["spread"]["%s.m%s.%s" % (side, m, key)] = round((max(v) - min(v)) / med(v), 4)
    md = out["median"]
    out["ratio"] = {"branch_m1_over_parent_m1.wall": round(md["branch.m1.wall_ms"] / md["parent.m1.wall_ms"], 4),
                    "branch_m1_over_parent_m1.sort": round(md["branch.m1.sort_ms"] / md["parent.m1.sort_ms"], 4)}
    if "2" in a.m.split(","):
        out["ratio"].update({"sort_m2_over_parent_sort_m1": round(md["branch.m2.sort_ms"] / md["parent.m1.sort_ms"], 4),
                             "kmer_m2_over_m1": round(md["branch.m2.kmer_ms"] / md["branch.m1.kmer_ms"], 4),
                             "encode_m2_over_m1": round(md["branch.m2.encode_ms"] / md["branch.m1.encode_ms"], 4),
                             "sort_share_of_step_m2": round(md["branch.m2.sort_ms"] / (md["branch.m2.kmer_ms"] + md["branch.m2.sort_ms"] +
                                                                                        md["branch.m2.encode_ms"]), 4)})
    return out


if __name__ == "__main__":
    args = parse()
    print(json.dumps(compare(args) if args.parent_tree else measure(args)))
