"""The ANI matrix as text (libhypergen_tri.so) against hg_dist_full_dev run over the same row blocks of the same sketches: what the
format -- tri_format_kernel behind every block -- costs on top of the comparison it needs, what the trip over the host link
costs on top of that, and the command line end to end.  Input: the bench's clustered hypervectors (bench.clustered_hvs: clusters
of 100 members, ~96-97 % ANI inside a cluster, 0 across), D = 4096, Mash for HG_TRI_LOWER and containment for HG_TRI_FULL.
Legs per size and layout:
    dist_full_blocks  hg_dist_full_dev over the blocks hg_tri_dev cuts (LOWER: only the columns in front of a block's last row)
    tri_dev           hg_tri_dev, the text resident on the device
    tri_stream        hg_tri_stream_dev into a sink that discards
    cli               `hyper-gen triangle` on a .sketch file of the same hypervectors, -o on the file system of the run
The three library legs alternate in one process, --rounds times; each leg of a round is the median wall ms of --steps calls
(every call returns with its results final).  The command line runs --rounds times behind them.  Every case -- one size -- runs
in a child process of its own under its own time limit, and a case that fails or runs out of time ends the run: nothing more is
started.  Prints one JSON line and writes it to profiles/tri_bench.json.  No ratio is a pass condition.

    python tools/tri_bench.py [--n 10000 30000] [--rounds 3 --steps 3 --warmup 1] [--case-timeout 420] [--no-cli] [--no-write]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "tri_bench.json")
BLOCK_BYTES = 256 << 20  # HG_SEARCH_BLOCK_BYTES
HV_D = 4096
# written down before any run on an MI355X
EXPECTATION = ("tri_format_kernel is bound by 4 bytes read and 8 written per pair; at the 3.3 TB/s cluster_stats_rows_kernel reads at, "
               "30 000 x 30 000 pairs (10.8 GB) take 3.3 ms next to a 14.3 ms comparison: tri_dev a few per cent to a quarter above "
               "dist_full_blocks; tri_stream bound by the host link (7.2 GB of text at about 50 GB/s: 0.15 s); cli bound by the file system")


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


def rows_per_block(n):
    """rows_per_block of hg_tri.hip for hg_tri_dev"""
    fit = max(1, BLOCK_BYTES // (4 * n))
    if fit >= 256:
        fit -= fit % 256
    return min(n, fit)


def write_db(hg, np, path, hv):
    n2 = (hv.astype(np.int64) ** 2).sum(1).astype(np.int32)
    recs = []
    for i in range(hv.shape[0]):
        q, packed = hg.hv_pack(hv[i])
        recs.append(dict(ksize=21, scaled=1500, canonical=True, seed=123, hv_d=hv.shape[1], hv_quant_bits=q, hv_norm_2=int(n2[i]),
                         file_str="/data/genomes/cluster%04d/genome_%06d.fna" % (i // 100, i), hv=packed.view(np.int16)))
    hg.write_sketch_file(path, recs)


def run_case(a):
    """one size, in this process: the rows of the result"""
    import numpy as np
    import torch
    import hypergen_amd as hg
    import bench
    n = int(a.case)
    dev = torch.device("cuda:0")
    hv = bench.clustered_hvs(n, 0, dev)
    n2 = (hv.int() ** 2).sum(1).int()
    rb = rows_per_block(n)
    blk = torch.empty(rb * n, dtype=torch.float32, device=dev)
    discard = hg.TRI_SINK(lambda user, text, nbytes, row0, rows: 0)
    L = hg.lib_tri()
    rows = []
    with hg.Context(0) as c:
        for layout, name, metric in ((hg.TRI_LOWER, "lower", hg.ANI_MASH), (hg.TRI_FULL, "full", hg.ANI_CONTAINMENT)):
            c.set_ani_metric(metric)
            size = hg.tri_text_bytes(layout, 0, n, n)
            text = torch.empty(size, dtype=torch.uint8, device=dev)

            def dist_blocks():
                for r0 in range(0, n, rb):
                    r = min(rb, n - r0)
                    cols = r0 + r - 1 if layout == hg.TRI_LOWER else n
                    if cols:
                        c.dist_full_dev(hv.data_ptr() + 2 * r0 * HV_D, n2.data_ptr() + 4 * r0, r, hv.data_ptr(), n2.data_ptr(), cols, HV_D, 21, blk.data_ptr())
                c.sync()

            def tri_dev():
                c.tri_dev(hv.data_ptr(), n2.data_ptr(), n, HV_D, 21, layout, text.data_ptr())

            def tri_stream():
                c._ck(L.hg_tri_stream_dev(c._h, hv.data_ptr(), n2.data_ptr(), n, HV_D, 21, layout, 0, discard, None))

            legs = {"dist_full_blocks": dist_blocks, "tri_dev": tri_dev, "tri_stream": tri_stream}
            torch.cuda.synchronize()
            for fn in legs.values():
                for _ in range(a.warmup):
                    fn()
            per = {k: [] for k in legs}
            for _ in range(a.rounds):
                for k, fn in legs.items():
                    per[k].append(median_ms(fn, a.steps))
            row = {"n": n, "layout": name, "metric": "mash" if metric == hg.ANI_MASH else "containment", "block_rows": rb, "text_bytes": size}
            for k in legs:
                row[k] = summary(per[k])
            d = row["dist_full_blocks"]["median_ms"]
            row["tri_dev_over_dist"] = round(row["tri_dev"]["median_ms"] / d, 3)
            row["tri_stream_over_dist"] = round(row["tri_stream"]["median_ms"] / d, 3)
            row["tri_stream_gb_per_s"] = round(size / row["tri_stream"]["median_ms"] / 1e6, 2)
            del text
            rows.append(row)
    if not a.no_cli:
        with tempfile.TemporaryDirectory() as td:
            db, out = os.path.join(td, "db.sketch"), os.path.join(td, "out.phy")
            write_db(hg, np, db, hv.cpu().numpy())
            for row in rows:
                ts = []
                for _ in range(a.rounds):
                    t0 = time.perf_counter()
                    subprocess.run([hg.CLI_PATH, "triangle", "-p", db, "-o", out, "--ani_metric", row["metric"]], check=True, capture_output=True,
                                   timeout=a.case_timeout)
                    ts.append((time.perf_counter() - t0) * 1e3)
                row["cli"] = summary(ts)
                row["cli_file_bytes"] = os.path.getsize(out)
                os.remove(out)
    print("CASE " + json.dumps(rows), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[10_000, 30_000])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--case-timeout", type=int, default=420, help="seconds one child process may take")
    ap.add_argument("--no-cli", action="store_true", help="leave out the command-line leg")
    ap.add_argument("--no-write", action="store_true")
    ap.add_argument("--case", default=None, metavar="N", help="run one case in this process (what the parent starts)")
    a = ap.parse_args()
    if a.case:
        return run_case(a)
    rows, status = [], "measured"
    for n in a.n:
        cmd = [sys.executable, os.path.abspath(__file__), "--case", str(n), "--rounds", str(a.rounds), "--steps", str(a.steps), "--warmup", str(a.warmup),
               "--case-timeout", str(a.case_timeout)] + (["--no-cli"] if a.no_cli else [])
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.case_timeout)
        except subprocess.TimeoutExpired:
            status = "stopped: n = %d ran into its time limit of %d s" % (n, a.case_timeout)
            break
        got = [ln[5:] for ln in r.stdout.splitlines() if ln.startswith("CASE ")]
        if r.returncode != 0 or len(got) != 1:
            status = "stopped: n = %d ended with status %d: %s" % (n, r.returncode, r.stderr.strip().splitlines()[-1:] or "")
            break  # (whatever went wrong on the device: nothing more is started on it)
        rows += json.loads(got[0])
    out = {"bench": "tri", "status": status, "expectation": EXPECTATION, "rounds": a.rounds, "steps": a.steps, "cases": rows}
    line = json.dumps(out)
    if not a.no_write:
        with open(OUT, "w") as f:
            f.write(line + "\n")
    print(line)
    return 0 if status == "measured" else 1


if __name__ == "__main__":
    sys.exit(main())
