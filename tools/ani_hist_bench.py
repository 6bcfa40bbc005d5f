"""hg_hist_dev against hg_dist_full_dev run over the same row blocks of the same sketches: what the count -- hist_count_kernel over
every block -- costs on top of the comparison it needs.  Two inputs per size: the bench's clustered hypervectors
(bench.clustered_hvs: clusters of 100 members, ~96-97 % ANI inside a cluster, 0 across: every pair falls into a few dozen bins) and
unrelated random ones of the same size (about half of the pairs read exactly 0, the rest spread over the noise floor).  Per
input: HG_HIST_ALL and HG_HIST_UPPER at w = 100 (1 001 bins, four copies of the table, the block read once) and w = 1 (100 001
bins in 13 slices, the block read 13 times).  The legs alternate in one process, --rounds times; each leg of a round is the
median wall ms of --steps calls (every call returns with its results final).  The dist leg of HG_HIST_UPPER computes what the
histogram computes: only the columns from the block's first row on.  Every case -- one input at one size -- runs in a child
process of its own under its own time limit, and a case that fails or runs out of time ends the run: nothing more is started.
Prints one JSON line and writes it to profiles/ani_hist_bench.json.  No ratio is a pass condition.

    python tools/ani_hist_bench.py [--n 10000 30000] [--rounds 3 --steps 3 --warmup 1] [--case-timeout 240] [--no-write]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "ani_hist_bench.json")
BLOCK_BYTES = 256 << 20  # HG_SEARCH_BLOCK_BYTES
HV_D = 4096


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


def random_hvs(torch, rows, hashes=3333, seed=1):
    g = torch.Generator(device="cuda:0")
    g.manual_seed(seed)
    hv = torch.empty((rows, HV_D), dtype=torch.int16, device="cuda:0")
    for r0 in range(0, rows, 8192):  # (in slices: the float32 draw of all rows at once would double the footprint)
        r1 = min(rows, r0 + 8192)
        hv[r0:r1] = torch.round(hashes ** 0.5 * torch.randn((r1 - r0, HV_D), generator=g, device="cuda:0")).to(torch.int16)
    return hv


def run_case(a):
    """one input at one size, in this process: the rows of the result"""
    import torch
    import hypergen_amd as hg
    import bench
    kind, n = a.case[0], int(a.case[1])
    dev = torch.device("cuda:0")
    hv = bench.clustered_hvs(n, 0, dev) if kind == "clustered" else random_hvs(torch, n)
    n2 = (hv.int() ** 2).sum(1).int()
    rb = max(1, min(n, BLOCK_BYTES // (4 * n)))
    blk = torch.empty(rb * n, dtype=torch.float32, device=dev)
    rows = []
    with hg.Context(0) as c:
        for pairs, name in ((hg.HIST_ALL, "all"), (hg.HIST_UPPER, "upper")):
            def dist_blocks():
                for r0 in range(0, n, rb):
                    r, q0 = min(rb, n - r0), (r0 if pairs == hg.HIST_UPPER else 0)
                    c.dist_full_dev(hv.data_ptr() + 2 * r0 * HV_D, n2.data_ptr() + 4 * r0, r, hv.data_ptr() + 2 * q0 * HV_D, n2.data_ptr() + 4 * q0,
                                    n - q0, HV_D, 21, blk.data_ptr())
                c.sync()

            legs, tables = {"dist_full_blocks": dist_blocks}, {}
            for w in (100, 1):
                tables[w] = torch.zeros(hg.hist_bins(w) * 8, dtype=torch.uint8, device=dev)
                legs["hist_w%d" % w] = (lambda w=w: c.hist_dev(hv.data_ptr(), n2.data_ptr(), n, hv.data_ptr(), n2.data_ptr(), n, HV_D, 21, pairs, w,
                                                               tables[w].data_ptr()))
            torch.cuda.synchronize()
            for fn in legs.values():
                for _ in range(a.warmup):
                    fn()
            per = {k: [] for k in legs}
            for _ in range(a.rounds):
                for k, fn in legs.items():
                    per[k].append(median_ms(fn, a.steps))
            row = {"input": kind, "n": n, "pairs": name, "block_rows": rb}
            for k in legs:
                row[k] = summary(per[k])
            for w in (100, 1):
                counts = tables[w].cpu().numpy().view("<u8")
                row["hist_w%d_over_dist" % w] = round(row["hist_w%d" % w]["median_ms"] / row["dist_full_blocks"]["median_ms"], 3)
                row["bins_used_w%d" % w] = int((counts != 0).sum())
                row["share_in_bin_0_w%d" % w] = round(float(counts[0]) / float(counts.sum()), 4)
                assert int(counts.sum()) == (n * n if pairs == hg.HIST_ALL else n * (n - 1) // 2)
            rows.append(row)
    print("CASE " + json.dumps(rows), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[10_000, 30_000])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--case-timeout", type=int, default=240, help="seconds one child process may take")
    ap.add_argument("--no-write", action="store_true")
    ap.add_argument("--case", nargs=2, default=None, metavar=("INPUT", "N"), help="run one case in this process (what the parent starts)")
    a = ap.parse_args()
    if a.case:
        return run_case(a)
    rows, status = [], "measured"
    for n in a.n:
        for kind in ("clustered", "random"):
            cmd = [sys.executable, os.path.abspath(__file__), "--case", kind, str(n), "--rounds", str(a.rounds), "--steps", str(a.steps),
                   "--warmup", str(a.warmup)]
            try:
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.case_timeout)
            except subprocess.TimeoutExpired:
                status = "stopped: %s at n = %d ran into its time limit of %d s" % (kind, n, a.case_timeout)
                break
            got = [ln[5:] for ln in r.stdout.splitlines() if ln.startswith("CASE ")]
            if r.returncode != 0 or len(got) != 1:
                status = "stopped: %s at n = %d ended with status %d: %s" % (kind, n, r.returncode, r.stderr.strip().splitlines()[-1:] or "")
                break
            rows += json.loads(got[0])
        if status != "measured":
            break  # (whatever went wrong on the device: nothing more is started on it)
    out = {"bench": "ani_hist", "status": status, "rounds": a.rounds, "steps": a.steps, "cases": rows}
    line = json.dumps(out)
    if not a.no_write:
        with open(OUT, "w") as f:
            f.write(line + "\n")
    print(line)
    return 0 if status == "measured" else 1


if __name__ == "__main__":
    sys.exit(main())
