"""hg_frag_ani_dev against hg_dist_full_dev run over the same row blocks of the same hypervectors: what the reduction --
frag_best_kernel over every block, frag_fold_kernel behind every group of reference genomes -- costs on top of the comparison
it needs.  The sketches are unrelated random genomes: --ref_genomes genomes of --ref_windows windows of 2 x --hashes hashes
against --qry_genomes genomes of --qry_fragments fragments of --hashes hashes (a hypervector is normal(0, hashes) rounded per
dimension, which is all the ANI arithmetic sees of a sum of +-1 vectors), D = 4096, containment, k = 21.  The two legs alternate
in one process, --rounds times; each leg of a round is the median wall ms of --steps calls (every call returns with its
results final).  Since no fragment has a true match, every matched (reference genome, fragment) is a false one: their share
is reported at --fragment_ani 88, 90 and 92, with the largest best.  Prints one JSON line and writes it to
profiles/frag_ani_bench.json.  No ratio is a pass condition.

    python tools/frag_ani_bench.py [--ref_genomes 100 --ref_windows 1700 --qry_genomes 100 --qry_fragments 850]
                                   [--rounds 3 --steps 1 --warmup 1] [--no-write]

The best kernel's rate comes from a run of its own under the profiler, which writes nothing,

    rocprofv3 --kernel-trace --stats -d DIR -o stats --output-format csv -- python tools/frag_ani_bench.py --profiled [shape]

and is merged into the committed file afterwards:

    python tools/frag_ani_bench.py --merge-kernel-stats DIR/.../stats_kernel_stats.csv [shape]
"""
import argparse
import csv
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "frag_ani_bench.json")
BLOCK_BYTES = 256 << 20  # HG_SEARCH_BLOCK_BYTES
MAX_BLOCK_ROWS = 32768   # the rows hg_frag_ani_dev takes per block at the most
HV_D, KSIZE = 4096, 21
PROFILED_CALLS = 2


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


def random_hvs(torch, rows, hashes, seed):
    g = torch.Generator(device="cuda:0")
    g.manual_seed(seed)
    hv = torch.empty((rows, HV_D), dtype=torch.int16, device="cuda:0")
    for r0 in range(0, rows, 8192):  # (in slices: the float32 draw of all rows at once would double the footprint)
        r1 = min(rows, r0 + 8192)
        hv[r0:r1] = torch.round(hashes ** 0.5 * torch.randn((r1 - r0, HV_D), generator=g, device="cuda:0")).to(torch.int16)
    return hv, (hv.int() ** 2).sum(1).int()


def setup(torch, a):
    import numpy as np
    R, Q = a.ref_genomes * a.ref_windows, a.qry_genomes * a.qry_fragments
    rh, rn = random_hvs(torch, R, 2 * a.hashes, 1)
    qh, qn = random_hvs(torch, Q, a.hashes, 2)
    rf = np.arange(a.ref_genomes + 1, dtype=np.uint32) * a.ref_windows
    qf = np.arange(a.qry_genomes + 1, dtype=np.uint32) * a.qry_fragments
    torch.cuda.synchronize()
    return R, Q, rh, rn, qh, qn, rf, qf


def measure(c, hg, torch, a):
    import numpy as np
    R, Q, rh, rn, qh, qn, rf, qf = setup(torch, a)
    rb = max(1, min(R, MAX_BLOCK_ROWS, BLOCK_BYTES // (4 * Q)))
    blk = torch.empty(rb * Q, dtype=torch.float32, device="cuda:0")
    d_pair = torch.zeros(a.ref_genomes * a.qry_genomes * 16, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()

    def dist_blocks():
        for r0 in range(0, R, rb):
            r = min(rb, R - r0)
            c.dist_full_dev(rh.data_ptr() + 2 * r0 * HV_D, rn.data_ptr() + 4 * r0, r, qh.data_ptr(), qn.data_ptr(), Q, HV_D, KSIZE, blk.data_ptr())
        c.sync()

    def frag(th=90.0):
        c.frag_ani_dev(rh.data_ptr(), rn.data_ptr(), R, qh.data_ptr(), qn.data_ptr(), Q, HV_D, KSIZE, rf, qf, th, d_pair.data_ptr())

    legs = {"dist_full_blocks": dist_blocks, "frag_ani": frag}
    for fn in legs.values():
        for _ in range(a.warmup):
            fn()
    per = {k: [] for k in legs}
    for _ in range(a.rounds):
        for k, fn in legs.items():
            per[k].append(median_ms(fn, a.steps))
    out = {k: summary(v) for k, v in per.items()}
    out["frag_over_dist"] = round(out["frag_ani"]["median_ms"] / out["dist_full_blocks"]["median_ms"], 3)
    out["matrix_bytes"] = R * Q * 4
    out["block_rows"] = rb
    # every genome is unrelated to every other: a matched fragment is a false match
    false = {}
    for th in (88.0, 90.0, 92.0):
        frag(th)
        pair = d_pair.cpu().numpy().view(hg.FRAG_PAIR_DTYPE)
        false["%g" % th] = {"matched": int(pair["matched"].sum()), "of": int(a.ref_genomes) * Q,
                            "share": float(pair["matched"].sum()) / (a.ref_genomes * Q)}
    d_best = torch.zeros(a.ref_genomes * Q * 8, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    c.frag_ani_dev(rh.data_ptr(), rn.data_ptr(), R, qh.data_ptr(), qn.data_ptr(), Q, HV_D, KSIZE, rf, qf, 90.0, d_pair.data_ptr(), d_best.data_ptr())
    best = d_best.cpu().numpy().view(hg.FRAG_BEST_DTYPE)
    out["false_matches"] = false
    out["largest_unrelated_best"] = float(best["m"].max()) / 1000.0
    out["median_unrelated_best"] = float(np.median(best["m"])) / 1000.0
    return out


def profiled(c, torch, a):
    R, Q, rh, rn, qh, qn, rf, qf = setup(torch, a)
    d_pair = torch.zeros(a.ref_genomes * a.qry_genomes * 16, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    for _ in range(PROFILED_CALLS):
        c.frag_ani_dev(rh.data_ptr(), rn.data_ptr(), R, qh.data_ptr(), qn.data_ptr(), Q, HV_D, KSIZE, rf, qf, 90.0, d_pair.data_ptr())


def merge_kernel_stats(path, a):
    rows = {}
    with open(path) as f:
        for r in csv.DictReader(f):
            for k in ("frag_best_kernel", "frag_fold_kernel"):
                if k in r.get("Name", ""):
                    rows[k] = (float(r["TotalDurationNs"]), int(r["Calls"]))
    if "frag_best_kernel" not in rows:
        sys.exit("no frag_best_kernel row in %s" % path)
    matrix_bytes = PROFILED_CALLS * a.ref_genomes * a.ref_windows * a.qry_genomes * a.qry_fragments * 4
    out = json.load(open(OUT))
    out["kernels"] = {k: {"launches": n, "total_ms": round(ns / 1e6, 3)} for k, (ns, n) in rows.items()}
    out["kernels"]["frag_best_kernel"]["matrix_bytes_per_s"] = round(matrix_bytes / (rows["frag_best_kernel"][0] / 1e9), -6)
    out["kernels"]["source"] = "rocprofv3 --kernel-trace --stats of %d hg_frag_ani_dev calls, a run of its own" % PROFILED_CALLS
    line = json.dumps(out)
    with open(OUT, "w") as f:
        f.write(line + "\n")
    print(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref_genomes", type=int, default=100)
    ap.add_argument("--ref_windows", type=int, default=1700)
    ap.add_argument("--qry_genomes", type=int, default=100)
    ap.add_argument("--qry_fragments", type=int, default=850)
    ap.add_argument("--hashes", type=int, default=100, help="hashes of a query fragment; a reference window holds twice as many")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=1)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--no-write", action="store_true")
    ap.add_argument("--profiled", action="store_true", help="only run the calls a profiler traces")
    ap.add_argument("--merge-kernel-stats", default=None, help="a rocprofv3 kernel stats CSV of a --profiled run of the same shape")
    a = ap.parse_args()
    if a.merge_kernel_stats:
        return merge_kernel_stats(a.merge_kernel_stats, a)
    import torch
    import hypergen_amd as hg
    hg.lib_frag()
    with hg.Context(0) as c:
        c.set_ani_metric(hg.ANI_CONTAINMENT)
        if a.profiled:
            return profiled(c, torch, a)
        res = measure(c, hg, torch, a)
    out = {"bench": "frag_ani", "status": "measured", "rounds": a.rounds, "steps": a.steps,
           "shape": {"ref_genomes": a.ref_genomes, "ref_windows": a.ref_windows, "qry_genomes": a.qry_genomes, "qry_fragments": a.qry_fragments,
                     "hashes": a.hashes, "hv_d": HV_D, "ksize": KSIZE, "metric": "containment"}}
    out.update(res)
    line = json.dumps(out)
    if not a.no_write:
        with open(OUT, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
